"""vdb_index_search_hybrid_sum through the layers: the header declares it, the binding lists and types
it, the cross-compiled library exports it, and NativeIndex has its methods.  No compute calls (runs
without a GPU)."""
import inspect
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "vdb_index_search_hybrid_sum"


def test_the_header_declares_the_call_with_its_arguments():
    src = open(os.path.join(ROOT, "include", "vdb.h")).read()
    m = re.search(r"int32_t\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m, "no declaration"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["vdb_index* idx", "const float* queries", "const int64_t* q_indptr", "const int32_t* q_terms",
                    "const float* q_weights", "int32_t n_queries", "int64_t q_nnz", "int32_t k", "double w_dense",
                    "double w_sparse", "const uint32_t* row_mask", "int32_t mem", "float* out_scores",
                    "int64_t* out_indices", "double* out_fused", "double* out_dense", "double* out_sparse",
                    "int64_t index_offset", "void* stream"]
    for word in ("hybrid_sum_wgs", "hybrid_sum_searches", "hybrid_sum_queries"):
        assert word in src, word


def test_the_binding_lists_and_types_it():
    from service import _vdb
    assert NAME in _vdb.EXPORTED_SYMBOLS
    assert _vdb.HYBRID_SUM_MAX_K == 1024
    lib = _vdb.load_library()
    f = getattr(lib, NAME)
    assert len(f.argtypes) == 19 and f.restype is not None


def test_the_library_exports_it():
    from service import _vdb
    data = open(_vdb.library_path(), "rb").read()
    assert NAME.encode() in data and b"gfx950" in data
    assert hasattr(_vdb.load_library(), NAME)


def test_native_index_has_the_methods():
    from service import _vdb
    sig = inspect.signature(_vdb.NativeIndex.search_hybrid_sum)
    assert list(sig.parameters)[1:] == ["queries", "q_indptr", "q_terms", "q_weights", "k", "weights", "row_mask",
                                        "with_fused", "with_parts", "index_offset"]
    assert sig.parameters["weights"].default == (1.0, 1.0)
    assert callable(_vdb.NativeIndex.search_hybrid_sum_device)
