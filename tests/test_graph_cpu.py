"""_graph on the CPU: the list-to-CSR symmetrisation against a literal dense construction, the torch function against the numpy
one, and row_ids / jump at their edges.  Everything is compared bit for bit."""
import numpy as np
import pytest

from cryo_ralib_amd import _graph, spectral, tsne, umap


def mutual(n, k):
    """every row lists its k cyclic successors; with k = n - 1 every pair is mutual"""
    return (np.arange(n)[:, None] + np.arange(1, k + 1)[None, :]) % n


def planted(n=64, k=7, lonely=37, seed=5):
    """random lists over the other rows in which no row lists `lonely`"""
    rng = np.random.RandomState(seed)
    idx = np.empty((n, k), np.int64)
    for i in range(n):
        others = np.array([j for j in range(n) if j != i and j != lonely])
        idx[i] = rng.permutation(others)[:k]
    assert not np.any(idx == lonely)
    return idx


def one_way(n=9, k=3):
    """row i lists i + 1 .. i + k (mod n) and 2 k < n: no edge has its reverse"""
    idx = mutual(n, k)
    listed = {(i, int(j)) for i in range(n) for j in idx[i]}
    assert not any((j, i) in listed for i, j in listed)
    return idx


CASES = {"n5_k1": lambda: mutual(5, 1), "n5_k4_all_mutual": lambda: mutual(5, 4), "n64_k7_planted": planted, "one_way": one_way}

COMBINES = {"sum": lambda a, b: a + b, "mean": lambda a, b: 0.5 * (a + b), "union": lambda a, b: a + b - a * b}


def values(idx, seed=3):
    return np.random.RandomState(seed).uniform(0.05, 0.95, idx.shape)


def dense(idx, val, combine):
    """(indptr, indices, values): W [n][n] from the list, W and W.T combined, the stored entries read back in row-major order"""
    n = idx.shape[0]
    W, stored = np.zeros((n, n)), np.zeros((n, n), bool)
    for i in range(n):
        for t, j in enumerate(idx[i]):
            W[i, j] = val[i, t]
            stored[i, j] = stored[j, i] = True
    S = combine(W, W.T)                 # an absent entry is 0; v + 0, 0 + v and v + 0 - v 0 are v exactly, in either order
    rows, cols = np.nonzero(stored)
    return np.concatenate([[0], np.cumsum(stored.sum(axis=1))]), cols, S[rows, cols]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("combine", sorted(COMBINES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_symmetrize_equals_the_dense_construction(case, combine):
    idx = CASES[case]()
    val = values(idx)
    indptr, indices, a, b = _graph.symmetrize_numpy(idx, val)
    want_ptr, want_cols, want = dense(idx, val, COMBINES[combine])
    assert indptr.dtype == np.int64 and indices.dtype == np.int64
    assert np.array_equal(indptr, want_ptr) and np.array_equal(indices, want_cols)
    assert same_bits(COMBINES[combine](a, b), want)


@pytest.mark.parametrize("case", sorted(CASES))
def test_each_module_applies_its_own_combine(case):
    idx = CASES[case]()
    val = values(idx)
    n = idx.shape[0]
    p = tsne._symmetrize_numpy(idx, val)
    want_ptr, want_cols, want = dense(idx, val, COMBINES["sum"])
    assert np.array_equal(p[0], want_ptr) and np.array_equal(p[1], want_cols) and p[0].dtype == p[1].dtype == np.int64
    assert same_bits(p[2], want / max(float(np.sum(want)), tsne.MACHINE_EPSILON))
    for fn, name in ((spectral._symmetrize_numpy, "mean"), (umap._union_numpy, "union")):
        got = fn(idx, val)
        want_ptr, want_cols, want = dense(idx, val, COMBINES[name])
        assert got[0].dtype == got[1].dtype == np.int32 and len(got[0]) == n + 1
        assert np.array_equal(got[0], want_ptr) and np.array_equal(got[1], want_cols) and same_bits(got[2], want)


def test_the_cases_hit_the_edges():
    """what the shapes are chosen for: all keys doubled, no key doubled, and a row that only the transposes fill"""
    _, _, _, b = _graph.symmetrize_numpy(mutual(5, 4), values(mutual(5, 4)))
    assert np.all(b != 0) and len(b) == 20
    indptr, _, _, b = _graph.symmetrize_numpy(one_way(), values(one_way()))
    assert np.all(b == 0) and len(b) == 2 * 9 * 3
    idx = planted()
    indptr, indices, a, b = _graph.symmetrize_numpy(idx, values(idx))
    assert indptr[38] - indptr[37] == 7 and np.all(b[indptr[37]:indptr[38]] == 0)
    assert np.all(b[indices == 37] == 0) and np.any(b != 0)


@pytest.mark.parametrize("index_dtype", ["int32", "int64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_torch_on_cpu_tensors_equals_numpy(case, index_dtype):
    import torch
    idx = CASES[case]().astype(index_dtype)
    val = values(idx)
    want = _graph.symmetrize_numpy(idx, val)
    got = _graph.symmetrize_torch(torch.from_numpy(idx), torch.from_numpy(val))
    assert all(t.device.type == "cpu" for t in got)
    for g, w in zip(got, want):
        assert same_bits(g.numpy(), w)


def test_row_ids_with_empty_rows():
    import torch
    for indptr in ([0, 2, 2, 5], [0, 3, 4, 4], [0, 0, 0, 1, 1], [0, 0]):
        indptr = np.asarray(indptr, np.int64)
        want = np.array([i for i in range(len(indptr) - 1) for _ in range(indptr[i + 1] - indptr[i])], np.int64)
        assert same_bits(_graph.row_ids_numpy(indptr), want)
        for dt in (torch.int32, torch.int64):
            assert same_bits(_graph.row_ids_torch(torch.from_numpy(indptr).to(dt)).numpy(), want)


def test_jump_on_a_chain_and_on_fixed_points():
    n = 37
    chain = np.maximum(np.arange(n) - 1, 0)                     # x -> x - 1: every node ends at 0 after ceil(log2 n) doublings
    assert same_bits(_graph.jump(chain), np.zeros(n, np.int64))
    ident = np.arange(n)
    assert _graph.jump(ident) is ident
    two = np.array([0, 0, 1, 3, 3, 4, 5])
    assert np.array_equal(_graph.jump(two), [0, 0, 0, 3, 3, 3, 3])
    assert np.array_equal(two, [0, 0, 1, 3, 3, 4, 5])           # the input is left as it was
    assert _graph.jump(np.zeros(0, np.int64)).shape == (0,)


def test_graph_imports_no_feature_module_at_module_level():
    import ast
    for node in ast.parse(open(_graph.__file__).read()).body:
        if isinstance(node, ast.ImportFrom):
            assert node.level == 0 or node.module == "_common", ast.dump(node)
        if isinstance(node, ast.Import):
            assert all(not a.name.startswith(("cryo_ralib_amd", "torch")) for a in node.names), ast.dump(node)
