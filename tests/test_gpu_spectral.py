"""Spectral embedding on the device (csrc/ralign_spectral.h behind spectral.embedding): the four entries entry by entry against
float64 restatements at the edges of their tiles, then whole solves on every pin of tests/golden/spectral_ref.npz, bitwise
repeatability call to call and stream to stream, the two-blob subset identity, clustering, and the C entries' rejections.

The kernels' tile constants (ralign_spectral.h): LANES = 16 lanes share a CSR row and ROWS = 16 rows a workgroup; a lane loads
UNROLL = 4 entries per trip, so 64 entries of a row are in flight; the dots run over RUN = 512 rows per run, 64 lanes wide, CT = 16
columns per workgroup and CW = 4 per wave; the update and the norm partials take UPD = 64 rows per workgroup; the Ritz kernel 256 rows
by RT = 4 columns.  u = 2^-53.

ra_spectral_spmv.  Both sides add the len_i products of row i, in two different orders, the device with one rounding per
fused multiply-add and the restatement with two: |y_i - ref_i| <= 2 (len_i + 1) u sum_p |val_p x_p|.

One ra_spectral_lanczos step, from a state (M, q0, v_0 .. v_j) built on the host and handed to both sides.  The operator of these
tests has rows of at most 3 entries, so a product row costs no more roundings than the 4 the bound allows.  Write |.| for the same
computation on magnitudes:
    m0_i = sum_p |M_ip| |v_j[p]|                                 the magnitudes behind w = M v_j
    A    = sum_i |v_j[i]| m0_i                                   ... behind alpha_j = v_j . w
    H_t  = sum_i |Q_t[i]| m_i,  m_i <- m_i + sum_t H_t |Q_t[i]|  ... behind one pass h = Q^T w, w -= Q h; run twice from m0: m2
Every quantity is a sum of at most n products (a dot) followed by at most j + 2 products and a subtraction (the update), each
rounded at most twice, on either side: with g = 2 (n + j + 4) u,
    |alpha - alpha'| <= g A,   |w_i - w'_i| <= g m2_i,   |beta - beta'| <= g |m2|_2   (| |w| - |w'| | <= |w - w'|),
    |v_i - v'_i| = |w_i / beta - w'_i / beta'| <= g (m2_i + |v'_i| |m2|_2) / beta'.
After the step |Q^T v_{j+1}| <= (n + j) 2^-52 entry by entry; Q, the earlier vectors and the vectors after v_{j+1} keep their bits.

ra_spectral_ritz: m products per entry in j order, fused on the device: |Y - ref| <= 2 (m + 1) u sum_j |S[j][t]| |V_j[i]|."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import spectral_cases as sc  # noqa: E402
from cryo_ralib_amd import api, spectral  # noqa: E402

U = 2.0 ** -53
LANES, ROWS, UNROLL, RUN, CT, CW, UPD, RT = 16, 16, 4, 512, 16, 4, 64, 4
TRIP = LANES * UNROLL
RA_ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def z():
    with np.load(sc.GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def cases():
    return sc.pin_cases()


@pytest.fixture(scope="module")
def checker(cases):
    return {c: spectral.embedding(X, backend="numpy", **opt) for c, (X, opt, _) in cases.items()}


@pytest.fixture(scope="module")
def solved(cases, dev):
    return {c: spectral.embedding(torch.from_numpy(X).to(dev), **opt) for c, (X, opt, _) in cases.items()}


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- ra_spectral_spmv

def spmv_case(lengths, n, seed):
    indptr, indices, val = sc.random_csr(lengths, n, seed)
    return indptr, indices, val, np.random.default_rng(seed + 1).normal(size=n)


def spmv_check(indptr, indices, val, x, dev):
    L = api.load_library()
    n = len(indptr) - 1
    ins = [up(indptr, dev), up(indices if len(indices) else np.zeros(1, np.int32), dev), up(val if len(val) else np.zeros(1), dev), up(x, dev)]
    before = [t.clone() for t in ins]
    y = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    assert L.ra_spectral_spmv(P(ins[0]), P(ins[1]), P(ins[2]), n, P(ins[3]), P(y), stream()) == 0, L.ra_last_error()
    got = y.cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(indptr))
    ref = np.bincount(rows, weights=val * x[indices], minlength=n)
    mag = np.bincount(rows, weights=np.abs(val * x[indices]), minlength=n)
    bound = 2.0 * (np.diff(indptr) + 1) * U * mag
    print("spmv n", n, "worst error / bound", float(np.max(np.where(bound > 0, np.abs(got - ref) / np.where(bound > 0, bound, 1), 0))))
    assert np.all(np.abs(got - ref) <= bound)
    assert np.all(got[np.diff(indptr) == 0] == 0.0)
    assert all(torch.equal(a, b) for a, b in zip(ins, before))


def test_spmv_row_lengths(dev):
    """row lengths 0, 1, one below / at / above the lane group, around one trip of the unroll (64 entries), and 300"""
    lengths = [0, 1, LANES - 1, LANES, LANES + 1, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1, 300]
    n = 320
    spmv_check(*spmv_case((lengths * 32)[:n], n, 3), dev)


@pytest.mark.parametrize("n", (1, 2, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1))
def test_spmv_rows_per_workgroup(dev, n):
    rng = np.random.default_rng(n)
    spmv_check(*spmv_case(rng.integers(0, n + 1, n), n, 5 + n), dev)


def test_spmv_refuses_a_column_out_of_range(dev):
    L = api.load_library()
    n = 40
    indptr, indices, val, x = spmv_case([3] * n, n, 9)
    for where, col in ((0, n), (57, -1), (len(indices) - 1, 2 ** 30)):
        bad = indices.copy()
        bad[where] = col
        y = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        rc = L.ra_spectral_spmv(P(up(indptr, dev)), P(up(bad, dev)), P(up(val, dev)), n, P(up(x, dev)), P(y), stream())
        assert rc == RA_ERR_ARG and b"ra_spectral_spmv" in L.ra_last_error()
        torch.cuda.synchronize()
        assert torch.all(y == -7.0)
    down = indptr.copy()
    down[5] = down[4] - 1
    y = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    assert L.ra_spectral_spmv(P(up(down, dev)), P(up(indices, dev)), P(up(val, dev)), n, P(up(x, dev)), P(y), stream()) == RA_ERR_ARG
    torch.cuda.synchronize()
    assert torch.all(y == -7.0)


# ---- one Lanczos step

def lanczos_state(n, j, seed):
    """a ring of n rows with a chord across from every third row of its first half (rows of 2 or 3 entries) and random weights:
    its _NumpyOperator, and a basis q0, v_0 .. v_j orthonormal to rounding"""
    rng = np.random.default_rng(seed)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    k = np.arange(0, n // 2, 3)
    indptr, indices, _ = sc.edges_to_csr(n, np.concatenate([ring, np.stack([k, k + n // 2], axis=1)]))
    assert np.diff(indptr).max() == 3 and np.diff(indptr).min() == 2
    rows = np.repeat(np.arange(n), np.diff(indptr))
    wgt = rng.uniform(0.5, 1.5, (n, n))
    a = 0.5 * (wgt[rows, indices] + wgt[indices, rows])
    op = spectral._NumpyOperator(indptr, indices, a)
    q0 = np.sqrt(op.deg) / np.sqrt(np.sum(op.deg))
    B, _ = np.linalg.qr(np.column_stack([q0, rng.normal(size=(n, j + 1))]))
    B = B * np.sign(B[:, 0] @ q0)
    return indptr, indices, op, q0, np.ascontiguousarray(B[:, 1:].T)


def lanczos_check(n, j, dev, seed=0):
    L = api.load_library()
    indptr, indices, op, q0, V = lanczos_state(n, j, seed + 31 * n + j)
    ldv, m_cap = n + 3, j + 3
    op.start(q0, V[0], m_cap)
    op.Q[1:j + 2] = V
    op.run(j, 1)
    alpha_c, beta_c, v_c = op.alpha[j], op.beta[j], op.Q[j + 2]
    Vd = torch.full((m_cap + 1, ldv), -7.0, dtype=torch.float64, device=dev)
    Vd[:j + 1, :n] = up(V, dev)
    before = Vd.clone()
    q0d, ab = up(q0, dev), torch.full((2, m_cap), -7.0, dtype=torch.float64, device=dev)
    ins = [up(indptr, dev), up(indices, dev), up(op.val, dev)]
    work = torch.empty(int(L.ra_spectral_work_bytes(n, j + 1)), dtype=torch.uint8, device=dev)
    assert work.numel() > 0 and work.data_ptr() % 256 == 0
    rc = L.ra_spectral_lanczos(P(ins[0]), P(ins[1]), P(ins[2]), n, P(q0d), P(Vd), ldv, j, 1, P(ab[0]), P(ab[1]), P(work), stream())
    assert rc == 0, L.ra_last_error()
    got, abh = Vd.cpu().numpy(), ab.cpu().numpy()
    # everything but row j + 1's first n entries keeps its bits
    keep = np.ones(got.shape, bool)
    keep[j + 1, :n] = False
    assert np.array_equal(got[keep], before.cpu().numpy()[keep]) and torch.equal(q0d, up(q0, dev))
    assert np.all(abh[:, np.arange(m_cap) != j] == -7.0)
    # the magnitudes of the docstring
    Q = np.abs(op.Q[:j + 2])
    m0 = np.bincount(op.rows, weights=np.abs(op.val) * np.abs(V[j])[op.indices], minlength=n)
    A, m2 = float(np.abs(V[j]) @ m0), m0.copy()
    for _ in range(2):
        m2 = m2 + (Q @ m2) @ Q
    g = 2.0 * (n + j + 4) * U
    v_d = got[j + 1, :n]
    nm2 = float(np.linalg.norm(m2))
    bound_v = g * (m2 + np.abs(v_c) * nm2) / beta_c
    print("lanczos n %d j %d: alpha %.3e / %.3e  beta %.3e / %.3e  v %.3e of its bound" % (
        n, j, abs(abh[0, j] - alpha_c), g * A, abs(abh[1, j] - beta_c), g * nm2, float(np.max(np.abs(v_d - v_c) / bound_v))))
    assert beta_c > 1e-3
    assert abs(abh[0, j] - alpha_c) <= g * A and abs(abh[1, j] - beta_c) <= g * nm2
    assert np.all(np.abs(v_d - v_c) <= bound_v)
    assert np.all(np.abs(op.Q[:j + 2] @ v_d) <= (n + j) * 2.0 * U)


@pytest.mark.parametrize("n", (UPD - 1, UPD, UPD + 1, RUN - 1, RUN, RUN + 1, 2 * RUN + UPD + 1))
def test_lanczos_step_rows(dev, n):
    """n around the update's 64 rows (the reduction of the norm partials' edge) and around the run length of the dots"""
    lanczos_check(n, CW + 1, dev)


@pytest.mark.parametrize("j", (0, 1, CW - 2, CW - 1, CT - 3, CT - 2, CT - 1, 2 * CT + 1))
def test_lanczos_step_basis_sizes(dev, j):
    """basis sizes 1 and 2, and Q = [q0, v_0 .. v_j] of j + 2 columns around the wave's 4 and the workgroup's 16 columns"""
    lanczos_check(RUN + 1, j, dev)


def test_lanczos_enqueues_steps_like_single_steps(dev):
    """steps = 5 in one call gives the bits of five calls of one step; a zero start breaks down cleanly (beta = 0, zeros)"""
    L = api.load_library()
    n, m = 300, 6
    indptr, indices, op, q0, V = lanczos_state(n, 0, 77)
    ins = [up(indptr, dev), up(indices, dev), up(op.val, dev), up(q0, dev)]
    work = torch.empty(int(L.ra_spectral_work_bytes(n, m)), dtype=torch.uint8, device=dev)
    outs = []
    for split in (False, True):
        Vd = torch.zeros((m + 1, n), dtype=torch.float64, device=dev)
        Vd[0] = up(V[0], dev)
        ab = torch.zeros((2, m), dtype=torch.float64, device=dev)
        for j0, steps in ([(j, 1) for j in range(5)] if split else [(0, 5)]):
            assert L.ra_spectral_lanczos(P(ins[0]), P(ins[1]), P(ins[2]), n, P(ins[3]), P(Vd), n, j0, steps, P(ab[0]), P(ab[1]), P(work),
                                         stream()) == 0, L.ra_last_error()
        outs.append((Vd.cpu().numpy(), ab.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    G = outs[0][0][:6] @ outs[0][0][:6].T
    assert np.all(np.abs(G - np.eye(6)) <= (n + 6) * 2.0 * U)
    Vd = torch.zeros((m + 1, n), dtype=torch.float64, device=dev)
    ab = torch.full((2, m), -7.0, dtype=torch.float64, device=dev)
    assert L.ra_spectral_lanczos(P(ins[0]), P(ins[1]), P(ins[2]), n, P(ins[3]), P(Vd), n, 0, 3, P(ab[0]), P(ab[1]), P(work), stream()) == 0
    assert torch.all(Vd == 0) and torch.all(ab[:, :3] == 0) and torch.all(ab[:, 3:] == -7.0)


# ---- ra_spectral_ritz

@pytest.mark.parametrize("n", (1, 255, 256, 257))
@pytest.mark.parametrize("m,c", ((1, 1), (2, RT - 1), (7, RT), (9, RT + 1), (40, 64)))
def test_ritz(dev, n, m, c):
    L = api.load_library()
    rng = np.random.default_rng(1000 * n + 10 * m + c)
    V, S, ldv = rng.normal(size=(m, n)), rng.normal(size=(m, c)), n + 5
    Vd = torch.full((m, ldv), -7.0, dtype=torch.float64, device=dev)
    Vd[:, :n] = up(V, dev)
    Sd, Y = up(S, dev), torch.full((c, n), -7.0, dtype=torch.float64, device=dev)
    before = Vd.clone()
    assert L.ra_spectral_ritz(P(Vd), ldv, m, n, P(Sd), c, P(Y), stream()) == 0, L.ra_last_error()
    got, ref, mag = Y.cpu().numpy(), S.T @ V, np.abs(S).T @ np.abs(V)
    assert np.all(np.abs(got - ref) <= 2.0 * (m + 1) * U * mag)
    assert torch.equal(Vd, before) and torch.equal(Sd, up(S, dev))


# ---- ra_spectral_components

def device_components(indptr, indices, dev):
    """(labels, rounds): the entry called until its one int says that nothing moved"""
    L = api.load_library()
    n = len(indptr) - 1
    ip, ix = up(indptr, dev), up(indices if len(indices) else np.zeros(1, np.int32), dev)
    label = torch.arange(n, dtype=torch.int32, device=dev)
    changed = torch.full((1,), -7, dtype=torch.int32, device=dev)
    for r in range(1, n + 2):
        assert L.ra_spectral_components(P(ip), P(ix), n, P(label), P(changed), stream()) == 0, L.ra_last_error()
        if int(changed.item()) == 0:
            return label.cpu().numpy().astype(np.int64), r
    raise AssertionError("the labels still move after n + 1 rounds")


def test_components(dev, z):
    graphs = {
        "path": sc.path_graph(2 * 256 + ROWS + 1)[:2],
        "two": sc.edges_to_csr(300, np.concatenate([np.stack([np.arange(0, 296, 2), np.arange(2, 298, 2)], 1),
                                                      np.stack([np.arange(1, 298, 2), np.arange(3, 300, 2)], 1), [[298, 0]]]))[:2],
        "isolated": sc.edges_to_csr(70, [(3, 60), (60, 17), (5, 6), (69, 0)])[:2],
        "none": (np.zeros(18, np.int32), np.zeros(0, np.int32)),
        "one_row": (np.zeros(2, np.int32), np.zeros(0, np.int32)),
        "one": (z["sk_indptr_gauss3"], z["sk_indices_gauss3"].astype(np.int32)),
    }
    for name, (indptr, indices) in graphs.items():
        got, rounds = device_components(indptr, indices, dev)
        want = spectral.components_numpy(indptr, indices)
        print("components", name, "rounds", rounds)
        assert np.array_equal(got, want), name
    assert len(np.unique(device_components(*graphs["two"], dev)[0])) == 2
    assert not device_components(*graphs["one"], dev)[0].any()


# ---- whole solves

@pytest.mark.parametrize("c", tuple(sc.pin_cases()))
def test_pin_embedding(dev, z, cases, checker, solved, c):
    X, opt, with_sklearn = cases[c]
    graph = spectral.graph(torch.from_numpy(X).to(dev), **sc.graph_options(opt))
    cpu = spectral.graph(X, backend="numpy", **sc.graph_options(opt))
    assert np.array_equal(graph[0], cpu[0]) and np.array_equal(graph[1], cpu[1]) and np.array_equal(graph[3], cpu[3])
    assert np.all(np.abs(graph[2] - cpu[2]) <= 8 * sc.EPS * cpu[2])
    if c not in ("selftune", "alpha1"):
        assert np.array_equal(graph[2], cpu[2])
    sc.check_against_pins(z, c, solved[c], graph, with_sklearn)
    dth = np.abs(solved[c].eigenvalues - checker[c].eigenvalues)
    print(c, "|theta - checker|", dth, "steps", solved[c].n_steps, checker[c].n_steps)
    assert np.all(dth <= solved[c].residuals + checker[c].residuals)


def test_same_bits_call_to_call_and_stream_to_stream(dev, cases, solved):
    X, opt, _ = cases["gauss5"]
    Xd = torch.from_numpy(X).to(dev)
    again = spectral.embedding(Xd, **opt)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = spectral.embedding(Xd, **opt)
    side.synchronize()
    for r in (again, other):
        assert np.array_equal(r.embedding, solved["gauss5"].embedding) and np.array_equal(r.eigenvalues, solved["gauss5"].eigenvalues)
        assert np.array_equal(r.residuals, solved["gauss5"].residuals) and r.n_steps == solved["gauss5"].n_steps


def test_two_blobs_embed_the_larger_one_bitwise(dev):
    X, first = sc.two_blobs(90, 150, 3, 7)
    with pytest.warns(spectral.SpectralWarning, match="Graph is not fully connected, spectral embedding may not work as expected.*90 rows"):
        res = spectral.embedding(torch.from_numpy(X).to(dev), 3, n_neighbors=8)
    alone = spectral.embedding(torch.from_numpy(np.ascontiguousarray(X[~first])).to(dev), 3, n_neighbors=8)
    assert res.n_dropped == 90 and np.array_equal(res.rows, np.nonzero(~first)[0])
    assert np.array_equal(res.embedding[~first], alone.embedding) and np.all(np.isnan(res.embedding[first]))
    assert np.array_equal(res.eigenvalues, alone.eigenvalues) and np.array_equal(res.residuals, alone.residuals)
    assert np.array_equal(res.component, np.where(first == first[0], 0, 1).astype(np.int32))


def test_cluster_equals_the_pinned_partition(dev, z):
    res = spectral.cluster(torch.from_numpy(z["arcs_X"]).to(dev), 2, n_neighbors=sc.ARCS["n_neighbors"])
    assert sc.same_partition(res.labels, z["arcs_labels"])
    also = api.spectral_cluster(z["arcs_X"], 2, n_neighbors=sc.ARCS["n_neighbors"])
    assert np.array_equal(also.labels, res.labels)


def test_embedding_from_graph_on_the_device(dev, cases, solved):
    X, opt, _ = cases["gauss3"]
    ip, ix, a, _ = spectral.graph(X, backend="numpy", n_neighbors=opt["n_neighbors"])
    res = spectral.embedding_from_graph(ip, ix, a, n_components=opt["n_components"])
    assert np.array_equal(res.embedding, solved["gauss3"].embedding)


def test_smallest_inputs_break_down_cleanly(dev):
    """n = 3 (the triangle: the complement of q0 is one eigenspace, beta_0 = 0) and a weighted path of 5 rows (complete at n_sub - 1 steps)"""
    X = np.array([[0.0, 0.0], [1.0, 0.25], [0.5, 2.0]], np.float32)
    res = spectral.embedding(torch.from_numpy(X).to(dev), 1, n_neighbors=3)
    assert res.converged and res.n_steps <= 2 and abs(res.eigenvalues[0] + 0.5) <= 4 * sc.EPS and res.residuals[0] <= 8 * sc.EPS
    assert np.all(np.isfinite(res.embedding)) and abs(res.embedding[:, 0].sum()) <= 8 * sc.EPS
    ip, ix, a = sc.weighted_path(5)
    res = spectral.embedding_from_graph(ip, ix, a, 3, drop_first=False, diffusion_time=2.0)
    E, theta, _, _ = spectral.dense_numpy(ip, ix, a, 3, drop_first=False, diffusion_time=2.0)
    assert res.converged and res.n_steps <= 4 and np.all(np.abs(res.eigenvalues - theta) <= 8 * sc.EPS)
    assert np.all(np.abs(res.embedding - E) <= 64 * sc.EPS)


def test_tool_on_the_device(dev, z, solved, tmp_path):
    x, o = str(tmp_path / "x.npy"), str(tmp_path / "out.npz")
    np.save(x, z["X_gauss3"])
    assert spectral.main([x, o, "--n_components", "5", "--n_neighbors", "10", "--k", "3", "--quality", "5"]) == 0
    with np.load(o) as f:
        assert np.array_equal(f["embedding"], solved["gauss3"].embedding) and np.array_equal(f["residuals"], solved["gauss3"].residuals)
        assert f["labels"].shape == (400,) and set(f["labels"]) == {0, 1, 2} and f["centers"].shape == (3, 3)
        assert int(f["n_steps"]) == solved["gauss3"].n_steps and bool(f["converged"]) and str(f["backend"]) == "device"
        assert 0.0 < float(f["trustworthiness"]) <= 1.0 and 0.0 < float(f["continuity"]) <= 1.0


def test_c_entries_reject(dev):
    L = api.load_library()
    n = 8
    ip = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=dev)
    ix = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    val, x, y = (torch.full((2 * n,), 7.0, dtype=torch.float64, device=dev) for _ in range(3))
    V = torch.full((4, n), 7.0, dtype=torch.float64, device=dev)
    ab = torch.full((2, 4), 7.0, dtype=torch.float64, device=dev)
    work = torch.full((1 << 16,), 7, dtype=torch.uint8, device=dev)
    lab = torch.full((n,), 7, dtype=torch.int32, device=dev)
    chg = torch.full((1,), 7, dtype=torch.int32, device=dev)
    s = stream()
    spmv, lan, ritz, comp = L.ra_spectral_spmv, L.ra_spectral_lanczos, L.ra_spectral_ritz, L.ra_spectral_components
    bad = [spmv(P(ip), P(ix), P(val), 0, P(x), P(y), s), spmv(P(ip), P(ix), P(val), 262145, P(x), P(y), s),
           spmv(None, P(ix), P(val), n, P(x), P(y), s), spmv(P(ip), None, P(val), n, P(x), P(y), s),
           spmv(P(ip), P(ix), None, n, P(x), P(y), s), spmv(P(ip), P(ix), P(val), n, None, P(y), s),
           spmv(P(ip), P(ix), P(val), n, P(x), None, s), spmv(P(ip), P(ix), P(val), n, P(x), P(x), s)]
    assert all(rc == RA_ERR_ARG for rc in bad), bad
    assert b"ra_spectral_spmv" in L.ra_last_error()

    def lanczos(n_=n, q0=x, V_=V, ldv=n, j0=0, steps=1, al=ab[0], be=ab[1], wk=work, ip_=ip, ix_=ix, val_=val, off=0):
        return lan(P(ip_), P(ix_), P(val_), n_, P(q0), P(V_), ldv, j0, steps, P(al), P(be),
                   ctypes.c_void_p(wk.data_ptr() + off) if wk is not None else None, s)

    bad = [lanczos(n_=1), lanczos(n_=262145), lanczos(ldv=n - 1), lanczos(j0=-1), lanczos(steps=0), lanczos(j0=4096), lanczos(j0=4000, steps=97),
           lanczos(steps=4097), lanczos(ip_=None), lanczos(ix_=None), lanczos(val_=None), lanczos(q0=None), lanczos(V_=None), lanczos(al=None),
           lanczos(be=None), lanczos(wk=None), lanczos(off=8)]
    assert all(rc == RA_ERR_ARG for rc in bad), bad
    assert b"ra_spectral_lanczos" in L.ra_last_error()
    assert L.ra_spectral_work_bytes(1, 4) == 0 and L.ra_spectral_work_bytes(n, 0) == 0 and L.ra_spectral_work_bytes(n, 4097) == 0
    bad = [ritz(P(V), n, 3, 0, P(x), 2, P(y), s), ritz(P(V), n, 3, 262145, P(x), 2, P(y), s), ritz(P(V), n - 1, 3, n, P(x), 2, P(y), s),
           ritz(P(V), n, 0, n, P(x), 2, P(y), s), ritz(P(V), n, 4097, n, P(x), 2, P(y), s), ritz(P(V), n, 3, n, P(x), 0, P(y), s),
           ritz(P(V), n, 3, n, P(x), 65, P(y), s), ritz(None, n, 3, n, P(x), 2, P(y), s), ritz(P(V), n, 3, n, None, 2, P(y), s),
           ritz(P(V), n, 3, n, P(x), 2, None, s)]
    assert all(rc == RA_ERR_ARG for rc in bad), bad
    assert b"ra_spectral_ritz" in L.ra_last_error()
    bad = [comp(P(ip), P(ix), 0, P(lab), P(chg), s), comp(P(ip), P(ix), 262145, P(lab), P(chg), s), comp(None, P(ix), n, P(lab), P(chg), s),
           comp(P(ip), None, n, P(lab), P(chg), s), comp(P(ip), P(ix), n, None, P(chg), s), comp(P(ip), P(ix), n, P(lab), None, s)]
    assert all(rc == RA_ERR_ARG for rc in bad), bad
    assert b"ra_spectral_components" in L.ra_last_error()
    torch.cuda.synchronize()
    assert torch.all(y == 7) and torch.all(V == 7) and torch.all(ab == 7) and torch.all(work == 7) and torch.all(lab == 7) and torch.all(chg == 7)
    # the python layer: errors before a launch
    Xd = torch.zeros((40, 3), device=dev)
    for f in (lambda: spectral.embedding(Xd, 0), lambda: spectral.embedding(Xd, 2, n_neighbors=41), lambda: spectral.embedding(Xd.double(), 2),
              lambda: spectral.embedding(Xd.t(), 2), lambda: spectral.embedding(Xd, 2, alpha=2.0), lambda: spectral.cluster(Xd, 1),
              lambda: spectral.embedding(torch.full((40, 3), float("nan"), device=dev), 2)):
        with pytest.raises(spectral.SpectralError):
            f()
