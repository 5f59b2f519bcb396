"""A batch at the automatic threshold of the integer-MFMA Hamming kernel through the store
(``batch_binary_query``): the same tuples as the queries issued one at a time (which take the popcount
kernel), and the index's "hamming_mfma_queries" rises by the batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, D, NB = 200, 16, 12
MIN_Q = 64  # csrc/vdb_hamming_plan.h kHamMfmaMinQueries


def test_batch_at_the_threshold_equals_single_queries(tmp_path):
    from service import _vdb, optimized_vector_store as sm
    assert _vdb.device_count() >= 1, "no GPU visible"
    rng = np.random.default_rng(4)
    X = rng.integers(0, 256, (N, NB), dtype=np.uint8)
    X[::4, 2:] = X[0, 2:]  # near duplicates: ties and near-ties at the head
    meta = [{"id": i, **({"code": X[i].tolist()} if i % 7 else {})} for i in range(N)]
    st = sm.MLXVectorStore(str(tmp_path / "s"), sm.MLXVectorStoreConfig(dimension=D, metric="cosine", persist=False))
    st.add_vectors(rng.standard_normal((N, D)).astype(np.float32), meta)
    Q = [q.tolist() for q in rng.integers(0, 256, (MIN_Q, NB), dtype=np.uint8)]
    singles = [st.binary_query(q, k=10) for q in Q]
    before = st._index.stat("hamming_mfma_queries")
    assert before == 0
    batch = st.batch_binary_query(Q, k=10)
    assert st._index.stat("hamming_mfma_queries") == before + MIN_Q
    assert batch == singles and all(len(t[0]) == 10 for t in batch)
