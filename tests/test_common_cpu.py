"""The layer the analysis modules share (cryo_ralib_amd/_common.py), without a GPU: every module refuses a bad input with its own
exception class and one text, the numpy backend's dtype rule per module, the file readers through their public bindings, the
truth scores when nothing is kept, and that the helpers exist once."""
import ast
import glob
import os

import numpy as np
import pytest

from cryo_ralib_amd import _common, dbscan, gmm, hdbscan, kmeans, sdr, tsne

PKG = os.path.dirname(os.path.abspath(_common.__file__))

# module, its error class, a call of its public entry with (X, backend)
MODULES = {
    "kmeans": (kmeans.KMeansError, lambda X, b: kmeans.kmeans(X, 2, random_state=0, backend=b)),
    "tsne": (tsne.TsneError, lambda X, b: tsne.tsne(X, perplexity=3.0, max_iter=250, random_state=0, backend=b)),
    "gmm": (gmm.GmmError, lambda X, b: gmm.gmm(X, 2, random_state=0, backend=b)),
    "dbscan": (dbscan.DbscanError, lambda X, b: dbscan.dbscan(X, 1.0, backend=b)),
    "hdbscan": (hdbscan.HdbscanError, lambda X, b: hdbscan.hdbscan(X, backend=b)),
}
ERRORS = [e for e, _ in MODULES.values()]


def points(n=12, d=3, dtype=np.float64):
    return np.random.RandomState(3).standard_normal((n, d)).astype(dtype)


def raises_own(name, X, backend, text):
    """the call raises the module's own class (and no other module's) with exactly `text`"""
    error, call = MODULES[name]
    with pytest.raises(error) as e:
        call(X, backend)
    assert type(e.value) is error and str(e.value) == text


@pytest.mark.parametrize("name", sorted(MODULES))
def test_bad_backend(name):
    raises_own(name, points(), "cuda", "backend is 'device' or 'numpy', got 'cuda'")


@pytest.mark.parametrize("name", sorted(MODULES))
def test_wrong_rank_on_the_numpy_backend(name):
    raises_own(name, points()[:, 0].copy(), "numpy", "X is [n][d], got shape (12,)")
    raises_own(name, points().reshape(2, 6, 3), "numpy", "X is [n][d], got shape (2, 6, 3)")


@pytest.mark.parametrize("name", sorted(MODULES))
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_value(name, value):
    X = points()
    X[7, 1] = value
    raises_own(name, X, "numpy", "X holds NaN or infinite values")


def test_tsne_takes_no_numpy_array_on_the_device_backend(monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("the device was touched before the input was refused")
    monkeypatch.setattr(torch.cuda, "current_device", touched)
    monkeypatch.setattr(torch.cuda, "current_stream", touched)
    raises_own("tsne", points(dtype=np.float32), "device", "backend 'device' takes a contiguous float32 CUDA tensor [n][d]")


@pytest.mark.parametrize("name", sorted(MODULES))
def test_device_backend_refuses_what_is_no_array(name):
    tail = "" if name == "tsne" else " (or a numpy array, copied)"
    raises_own(name, [[0.0, 1.0], [2.0, 3.0]], "device", "backend 'device' takes a contiguous float32 CUDA tensor [n][d]" + tail)


@pytest.mark.parametrize("name", ["dbscan", "hdbscan"])
def test_wrong_rank_numpy_array_is_refused_before_the_copy_to_the_device(name, monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("the device was touched before the input was refused")
    monkeypatch.setattr(torch.cuda, "current_device", touched)
    raises_own(name, points()[:, 0].copy(), "device", "X is [n][d], got shape (12,)")


class Stop(Exception):
    pass


@pytest.mark.parametrize("name,dtype", [("kmeans", np.float64), ("tsne", np.float64), ("gmm", np.float64), ("dbscan", np.float32),
                                        ("hdbscan", np.float32)])
def test_numpy_backend_dtype(name, dtype, monkeypatch):
    """dbscan and hdbscan get float32 (their rule 1), the others what they were given"""
    seen = []
    real = _common.as_input

    def spy(*a, **k):
        seen.append(real(*a, **k))
        raise Stop
    monkeypatch.setattr(_common, "as_input", spy)
    X = points(dtype=np.float64)
    with pytest.raises(Stop):
        MODULES[name][1](X, "numpy")
    assert len(seen) == 1 and isinstance(seen[0], np.ndarray) and seen[0].dtype == dtype
    assert np.array_equal(seen[0], X.astype(dtype))
    if dtype == np.float64:
        assert seen[0] is X


def test_as_input_copies_a_host_tensor_for_the_numpy_backend():
    import torch
    t = torch.arange(6, dtype=torch.float64).reshape(3, 2)
    got = _common.as_input(t, "numpy", ValueError)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, t.numpy())
    assert _common.as_input(t, "numpy", ValueError, numpy_dtype=np.float32).dtype == np.float32


def test_predicates():
    for v in (3, np.int32(3), np.int64(-1)):
        assert _common.is_int(v)
    for v in (True, np.bool_(False), 3.0, "3", None):
        assert not _common.is_int(v)
    for v in (1, 0.5, np.float32(2.0), np.int64(4)):
        assert _common.is_real(v)
    for v in (True, np.nan, np.inf, -np.inf, "1", None):
        assert not _common.is_real(v)


@pytest.mark.parametrize("module,error", [(kmeans, kmeans.KMeansError), (tsne, tsne.TsneError)])
def test_check_random_state(module, error):
    rs = np.random.RandomState(5)
    assert module.check_random_state(rs) is rs
    assert module.check_random_state(None) is np.random.mtrand._rand
    assert module.check_random_state(np.int64(7)).randint(1 << 30) == np.random.RandomState(7).randint(1 << 30)
    with pytest.raises(error) as e:
        module.check_random_state("seed")
    assert type(e.value) is error and str(e.value) == "random_state is None, an integer or a numpy RandomState, got 'seed'"


def test_gmm_refuses_a_bad_random_state_with_its_own_class():
    with pytest.raises(gmm.GmmError) as e:
        gmm.gmm(points(), 2, random_state=1.5, backend="numpy")
    assert type(e.value) is gmm.GmmError and str(e.value) == "random_state is None, an integer or a numpy RandomState, got 1.5"


# ---- the file readers through their public bindings

@pytest.mark.parametrize("module,error", [(kmeans, kmeans.KMeansError), (tsne, tsne.TsneError)])
def test_read_input(module, error, tmp_path):
    X = points(dtype=np.float64)
    np.save(tmp_path / "x.npy", X)
    np.savez(tmp_path / "x.npz", factors=X, other=X[:, :2])
    np.save(tmp_path / "flat.npy", X[:, 0])
    for got in (module.read_input(str(tmp_path / "x.npy")), module.read_input(str(tmp_path / "x.npz")),
                module.read_input(str(tmp_path / "x.npz"), "factors")):
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, X.astype(np.float32))
    assert module.read_input(str(tmp_path / "x.npz"), "other").shape == (12, 2)
    path = str(tmp_path / "x.npz")
    for args, text in (((path, "nope"), "%s: %s has no array 'nope' (it holds factors, other)" % (path, path)),
                       ((str(tmp_path / "flat.npy"),), "%s: need an [n][d] array, got shape (12,)" % (tmp_path / "flat.npy"))):
        with pytest.raises(error) as e:
            module.read_input(*args)
        assert type(e.value) is error and str(e.value) == text
    with pytest.raises(error) as e:
        module.read_input(str(tmp_path / "absent.npy"))
    assert type(e.value) is error and str(e.value).startswith("%s: " % (tmp_path / "absent.npy"))


def params_rows(n=6):
    rs = np.random.RandomState(2)
    order = rs.permutation(n)
    return np.stack([order, rs.uniform(0, 360, n), rs.uniform(-2, 2, n), rs.uniform(-2, 2, n), rs.randint(0, 2, n), order % 3], 1)


def test_read_truth(tmp_path):
    rows = params_rows()
    np.savetxt(tmp_path / "params.txt", rows, fmt="%d %.4f %.4f %.4f %d %d")
    np.save(tmp_path / "y.npy", np.arange(6, dtype=np.int32) % 3)
    np.save(tmp_path / "yf.npy", np.arange(6, dtype=np.float64))
    dup = rows.copy()
    dup[0, 0] = dup[1, 0]
    np.savetxt(tmp_path / "dup.txt", dup, fmt="%d %.4f %.4f %.4f %d %d")
    y = kmeans.read_truth(str(tmp_path / "params.txt"), 6)
    assert y.dtype == np.int64 and np.array_equal(y, np.arange(6) % 3)
    y = kmeans.read_truth(str(tmp_path / "y.npy"), 6)
    assert y.dtype == np.int64 and np.array_equal(y, np.arange(6) % 3)
    p = lambda f: str(tmp_path / f)
    for path, n, text in ((p("params.txt"), 5, "%s: need 5 rows of 6 columns (params.txt), got (6, 6)" % p("params.txt")),
                          (p("dup.txt"), 6, "%s: the idx column is not a permutation of 0 .. 5" % p("dup.txt")),
                          (p("y.npy"), 7, "%s: %s: need [7] integers, got int32 (6,)" % (p("y.npy"), p("y.npy"))),
                          (p("yf.npy"), 6, "%s: %s: need [6] integers, got float64 (6,)" % (p("yf.npy"), p("yf.npy")))):
        with pytest.raises(kmeans.KMeansError) as e:
            kmeans.read_truth(path, n)
        assert type(e.value) is kmeans.KMeansError and str(e.value) == text


def test_read_params(tmp_path):
    rows = params_rows()
    np.savetxt(tmp_path / "params.txt", rows, fmt="%d %.4f %.4f %.4f %d %d")
    np.savetxt(tmp_path / "init.txt", rows[:, 1:5], fmt="%.4f %.4f %.4f %d")
    np.savetxt(tmp_path / "five.txt", rows[:, :5], fmt="%d %.4f %.4f %.4f %d")
    got = sdr.read_params(str(tmp_path / "params.txt"), 6)
    want = np.empty((6, 4))
    want[rows[:, 0].astype(int)] = np.round(rows[:, 1:5], 4)
    assert got.shape == (6, 4) and np.allclose(got, want, atol=1e-12)
    assert np.allclose(sdr.read_params(str(tmp_path / "init.txt"), 6), np.round(rows[:, 1:5], 4), atol=1e-12)
    p = lambda f: str(tmp_path / f)
    for path, n, text in ((p("params.txt"), 7, "%s has 6 rows, the stack 7 images" % p("params.txt")),
                          (p("five.txt"), 6, "%s: rows of 5 columns; expected 6 (params.txt) or 4 (initial2Dparams.txt)" % p("five.txt"))):
        with pytest.raises(sdr.SdrError) as e:
            sdr.read_params(path, n)
        assert type(e.value) is sdr.SdrError and str(e.value) == text


# ---- the command lines' shared tail

def test_truth_scores():
    truth = np.array([0, 0, 1, 1, 2, 2])
    labels = np.array([1, 1, 0, 0, 0, -1], np.int32)
    out = {}
    text = _common.truth_scores(out, truth, labels)
    assert list(out) == ["purity", "c_purity", "contingency"]
    assert out["purity"] == kmeans.purity_score(truth, labels) and out["c_purity"] == kmeans.c_purity_score(truth, labels)
    assert np.array_equal(out["contingency"], kmeans.contingency_matrix(truth, labels))
    assert text == ", purity %.4f, c_purity %.4f" % (out["purity"], out["c_purity"])
    keep = labels >= 0
    kept = {}
    _common.truth_scores(kept, truth, labels, keep)
    assert kept["purity"] == kmeans.purity_score(truth[keep], labels[keep]) == 0.8
    assert np.array_equal(kept["contingency"], np.array([[0, 2], [2, 0], [1, 0]]))
    assert isinstance(kept["purity"], np.float64) and isinstance(kept["c_purity"], np.float64)


def test_truth_scores_with_nothing_kept():
    out = {}
    text = _common.truth_scores(out, np.arange(4), np.full(4, -1, np.int32), np.zeros(4, bool))
    assert isinstance(out["purity"], np.float64) and np.isnan(out["purity"])
    assert isinstance(out["c_purity"], np.float64) and np.isnan(out["c_purity"])
    assert out["contingency"].shape == (0, 0) and out["contingency"].dtype == np.int64
    assert text == ", purity nan, c_purity nan"


def test_ptr():
    assert _common.ptr(None) is None

    class T:
        def data_ptr(self):
            return 4096
    assert _common.ptr(T()).value == 4096


# ---- the helpers exist once

def sources():
    return sorted(glob.glob(os.path.join(PKG, "*.py")))


SHARED = ("_common", "_graph")          # the modules every feature module may import from


def test_no_module_imports_a_private_name_from_a_sibling():
    """`from .x import _name` and `from . import _x` are allowed only for the shared modules"""
    bad = []
    for path in sources():
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not isinstance(node, ast.ImportFrom) or not (node.level >= 1 or (node.module or "").startswith("cryo_ralib_amd")):
                continue
            source = (node.module or "").split(".")[-1]
            for a in node.names:
                if a.name.startswith("_") and not a.name.startswith("__") and a.name not in SHARED and source not in SHARED:
                    bad.append("%s: from %s import %s" % (os.path.basename(path), "." * node.level + (node.module or ""), a.name))
    assert not bad, bad


def test_the_shared_helpers_are_defined_once():
    """no module-level copy outside _common.py and _graph.py (Engine._ptr, a method that checks dtypes, is not one)"""
    names = {"_ptr", "_as_input", "_check_finite", "_is_int", "_is_real", "ptr", "as_input", "check_finite", "is_int", "is_real",
             "_host_finite", "host_finite", "_jump", "jump", "_row_ids", "_csr_rows", "row_ids_numpy", "row_ids_torch"}
    bad = []
    for path in sources():
        if os.path.basename(path)[:-3] in SHARED:
            continue
        for node in ast.parse(open(path).read(), path).body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name in names:
                bad.append("%s: def %s" % (os.path.basename(path), node.name))
    assert not bad, bad
    defined = {n.name for n in ast.parse(open(os.path.join(PKG, "_common.py")).read()).body if isinstance(n, ast.FunctionDef)}
    assert {"ptr", "as_input", "check_finite", "is_int", "is_real", "check_random_state", "read_input", "read_truth", "read_params",
            "add_cluster_arguments", "check_averages_arguments", "require_gpu", "to_device", "truth_scores", "write_averages",
            "host_finite"} <= defined


def test_common_imports_no_feature_module_at_module_level():
    for node in ast.parse(open(os.path.join(PKG, "_common.py")).read()).body:
        if isinstance(node, ast.ImportFrom):
            assert node.level == 0, ast.dump(node)
        if isinstance(node, ast.Import):
            assert all(not a.name.startswith(("cryo_ralib_amd", "torch")) for a in node.names), ast.dump(node)
