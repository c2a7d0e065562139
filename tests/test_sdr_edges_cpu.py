"""Input builders for the 2SDR kernels' tile, run and rank edges (tests/test_gpu_sdr_edges.py imports them), and the checks of the
builders themselves: every property a device case relies on is asserted here against numpy, without a GPU.

Integer builders.  Images are integers in -2 .. 2, the mean handed to the entries is an arbitrary integer pattern in -1 .. 1 (the
entries take any [p][q] array), projectors have entries in {-1, 0, 1}.  Every f32 product and every f32 partial sum the kernels
form is then an integer below 2^24, so it is exact whatever the order of the sum, and the device result must equal the numpy
result bit for bit.  The expected values are float64 matrix products of integers: every partial sum is an integer far below
2^53, so they are exact as well and equal the int64 products (test_float64_products_of_integers_equal_int64 checks that).

is_exact_* assert the condition per case from upper bounds of the sums of absolute values of the terms of each f32 accumulator:
    W entry                 sum_kk |P[kk][j]| |Xc[..]|              <= max column sum of |P| * max |Xc|
    per-run Gram partial    sum_rows |Z[row][a]| |Z[row][b]|        <= rows per run * (max |Z|)^2
    U entry                 sum_r |A[r][a]| |W1[b][r]|              <= max column sum of |A| * max column sum of |B| * max |Xc|
    F entry                 sum_t |U[i][t]| |G[t][c]|               <= max |U| * max column sum of |G|
Z is the row stream of the Gram (image rows, or the rows of W), rows per run follow the shape rule of ra_sdr_gram.

Sensitivity.  For each family the expected output changes when the contribution named by an edge is removed (the centred rows,
images or columns zeroed; a projector row or column zeroed), so no case is blind to the edge it is named for.

Real-valued bounds (u = 2^-24; every product is an f32 fma chain, one rounding per term, so a chain of L terms is off by at
most L u sum |terms| to first order; + 8 covers the second-order terms, the rounding of the f32 partial and the double combine):
    Gram entry      Z^T Z with Z = W (forms 1, 2) or the centred rows (form 0, K = 0).  A W entry is a chain of K terms (the
                    contracted length), so |dW| <= K u Wabs with Wabs = |P|^T |Xc| >= |W|.  A run's partial is a chain of N terms
                    (rows per run: k rows per image * images per run, or the stack rows of a form-0 run): N u sum |W_a| |W_b| of
                    its own rounding plus sum (|dW_a| |W_b| + |W_a| |dW_b|) <= 2 K u sum Wabs_a Wabs_b carried from W.  Summed over
                    the runs:   (N + 2 K + 8) u (Wabs^T Wabs)[a][b].
    U entry         W1[b][r] = sum_c B[c][b] Xc[r][c] is a chain of q terms: |dW1| <= q u W1abs, W1abs = |B|^T |Xc|^T.
                    U[a][b] = sum_r A[r][a] W1[b][r] is a chain of p terms: p u sum |A| |W1| of its own plus sum |A| |dW1|:
                                (p + q + 8) u (|A|^T |Xc| |B|)[a][b].
    F entry         one chain of m terms over the f32 U and G as given:   (m + 8) u (|U| |G|)[i][c].
    mean            double sums of n terms and one division, (n + 1) 2^-53 sum |x| / n, plus the one rounding to f32, u |mean|.
The soundness tests hold each bound between a float32 numpy evaluation of the same products (inside) and the same evaluation
with every operand cut to a 10-bit mantissa (outside)."""
import functools

import numpy as np
import pytest

U24 = 2.0 ** -24
U53 = 2.0 ** -53
LIMIT = 2.0 ** 24

SDR_RUN0_ROWS = 2048            # form 0: stack rows per run (whole images)
SDR_RUN_IMAGES = 32             # forms 1, 2: images per run
SDR_MEAN_RUN = 64               # images per partial of the mean


def run_images(form, p):
    """images per run of ra_sdr_gram"""
    return max(1, SDR_RUN0_ROWS // p) if form == 0 else SDR_RUN_IMAGES


def tile_geometry(d):
    """(nb, TD) of a d x d Gram: blocks per side and their width"""
    nb = (d + 127) // 128
    return nb, 16 * (((d + nb - 1) // nb + 15) // 16)


# ---- integer builders

def int_stack(n, p, q, seed=0):
    """float32 [n][p][q], integers in -2 .. 2; the corners of every image are non-zero"""
    rng = np.random.default_rng([n, p, q, seed])
    X = rng.integers(-2, 3, (n, p, q)).astype(np.float32)
    for r in (0, p - 1):
        for c in (0, q - 1):
            X[X[:, r, c] == 0, r, c] = 2.0
    return X


def int_mean(p, q, seed=0):
    """float32 [p][q], integers in -1 .. 1 in a non-constant pattern (any array serves as the mean of the entries)"""
    rng = np.random.default_rng([p, q, seed, 77])
    M = rng.integers(-1, 2, (p, q)).astype(np.float32)
    M[p - 1, q - 1] = -1.0
    M[0, 0] = 1.0 if p * q > 1 else -1.0
    return M


def int_proj(K, k, seed=0, nnz=4):
    """float32 [K][k], entries in {-1, 0, 1}: up to nnz non-zeros per column at random rows, and non-zeros in the first and last
    row and the first and last column (the four corners, and one more column of each of the two rows)"""
    rng = np.random.default_rng([K, k, seed, 99])
    M = np.zeros((K, k), np.float32)
    for j in range(k):
        rows = rng.choice(K, min(nnz, K), replace=False)
        M[rows, j] = rng.choice([-1.0, 1.0], len(rows))
    for r in (0, K - 1):
        for c in (0, k - 1, int(rng.integers(0, k))):
            if M[r, c] == 0:
                M[r, c] = rng.choice([-1.0, 1.0])
    return M


def centred(X, mean):
    """x - mean in float32, as the device forms it on load, widened to float64"""
    X = np.asarray(X, np.float32)
    return (X if mean is None else X - np.asarray(mean, np.float32)).astype(np.float64)


def w_stream(Xc, form, Pm=None):
    """the row stream Z of the Gram [rows][d]: the stack rows (form 0), the rows of W_i = P^T X_i^T (form 1) or P^T X_i (form 2)"""
    n, p, q = Xc.shape
    if form == 0:
        return Xc.reshape(n * p, q)
    Pm = np.asarray(Pm, np.float64)
    if form == 1:
        return np.matmul(Xc, Pm).transpose(0, 2, 1).reshape(-1, p)          # [n][k][p]
    return np.matmul(Pm.T, Xc).reshape(-1, q)                               # [n][k][q]


def gram_ref(Xc, form, Pm=None):
    """Z^T Z in float64"""
    Z = w_stream(Xc, form, Pm)
    return Z.T @ Z


def project_ref(Xc, A, B):
    """[n][p0 q0] float64, (a, b) -> a q0 + b"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.matmul(np.matmul(A.T, Xc), B).reshape(Xc.shape[0], -1)


def factors_ref(U, G):
    return np.asarray(U, np.float64) @ np.asarray(G, np.float64)


def mean_ref(X):
    """the per-pixel mean of integer images: the double sum is exact, one division, one rounding"""
    X = np.asarray(X, np.float64)
    return np.float32(X.sum(axis=0) / X.shape[0])


def is_integer_f32(*arrays):
    return all(a is None or (np.array_equal(a, np.rint(a)) and np.array_equal(np.asarray(a, np.float32).astype(np.float64),
                                                                               np.asarray(a, np.float64))) for a in arrays)


def is_exact_gram(X, mean, form, Pm=None):
    """every W entry and every per-run partial Gram entry the kernel forms is an integer sum whose absolute terms stay below 2^24"""
    n, p, q = X.shape
    Xc = centred(X, mean)
    if not is_integer_f32(X, mean, Pm):
        return False
    xmax = np.abs(Xc).max()
    zmax, k = xmax, p
    if form:
        wabs = np.abs(np.asarray(Pm, np.float64)).sum(axis=0).max() * xmax      # bounds the terms of a W entry and |W| itself
        if wabs >= LIMIT:
            return False
        zmax, k = wabs, Pm.shape[1]
    rows = min(n, run_images(form, p)) * k
    return bool(rows * zmax * zmax < LIMIT)


def is_exact_project(X, mean, A, B):
    if not is_integer_f32(X, mean, A, B):
        return False
    w1 = np.abs(np.asarray(B, np.float64)).sum(axis=0).max() * np.abs(centred(X, mean)).max()
    return bool(w1 < LIMIT and np.abs(np.asarray(A, np.float64)).sum(axis=0).max() * w1 < LIMIT)


def is_exact_factors(U, G):
    return is_integer_f32(U, G) and bool(np.abs(U).max() * np.abs(np.asarray(G, np.float64)).sum(axis=0).max() < LIMIT)


# ---- the cases (shapes only; the arrays come from the cached builders below)

MEAN_N = [1, 63, 64, 65, 1024, 1025]
MEAN_PQ = [(1, 1), (7, 9), (8, 8), (5, 13), (1, 255), (16, 16), (1, 257)]          # npix 1, 63, 64, 65, 255, 256, 257


def mean_cases():
    """(n, p, q): every n at npix 63 and 257, every npix at n = 65 and 1025"""
    cases = [(n, p, q) for n in MEAN_N for p, q in ((7, 9), (1, 257))]
    cases += [(n, p, q) for n in (65, 1025) for p, q in MEAN_PQ if (n, p, q) not in cases]
    return cases


GRAM0_D = [1, 15, 16, 17, 112, 113, 128, 129, 130, 160, 161, 255, 256]
GRAM0_TILE = [(7, 3 + 2 * (i % 2), d) for i, d in enumerate(GRAM0_D)]              # 21 or 35 stack rows: a partly filled last 16-row step
GRAM0_RUNS = [(n, 33, 17) for n in (61, 62, 63)] + [(n, 256, 17) for n in (8, 9, 128, 129, 136, 137)]
STAGE2_Q = [1, 127, 128, 129, 2047, 2048]
STAGE2_N = [1, 2047, 2048, 2049]
STAGE2 = ([(n, 1, q) for q in (129, 2048) for n in STAGE2_N] + [(2049, 1, 1), (2049, 1, 127), (2049, 1, 128), (17, 1, 2047),
          (16 * 2048 + 1, 1, 5)])

# (k, contracted length L, output side d): form 1 runs it on d x L images, form 2 on L x d images
GRAM12_KLD = [(1, 1, 16), (1, 17, 129), (3, 3, 17), (3, 33, 128), (4, 4, 16), (4, 47, 256), (5, 5, 129), (5, 90, 17),
              (15, 15, 128), (15, 255, 16), (16, 16, 256), (16, 17, 17), (17, 17, 16), (17, 256, 129), (33, 33, 17),
              (33, 47, 128), (48, 48, 129), (48, 90, 256), (49, 49, 16), (49, 255, 128), (64, 64, 17), (64, 90, 129),
              (64, 256, 256)]
GRAM12_K = [1, 3, 4, 5, 15, 16, 17, 33, 48, 49, 64]
GRAM12_L = [17, 33, 47, 90, 255, 256]
GRAM12_D = [16, 17, 128, 129, 256]
GRAM12_RUN_N = [1, 31, 32, 33, 512, 513, 544, 545, 1025]                           # 1, 1, 1, 2, 16, 17, 17, 18, 33 runs
GRAM12_NULL_MEAN_N = (33, 545)
GRAM12_RECT = [(33, 130), (130, 33)]

PROJECT_SIDES = [1, 15, 16, 17, 33, 48, 49, 64]
PROJECT_NAMED = [(64, 32), (32, 64), (1, 64), (64, 1), (17, 17), (49, 33)]
PROJECT_IMAGES = [None, (33, 47), (130, 129), (255, 256), (256, 255)]             # None: the image is p0 x q0 itself


def project_cases():
    """(n, p, q, p0, q0): every (p0, q0) of the grid with p0 q0 <= 2048 at one image shape (in rotation among those that hold it)
    and n 1 or 3 in turn; the named pairs at p0 x q0 itself and at one more"""
    cases = []
    grid = [(a, b) for a in PROJECT_SIDES for b in PROJECT_SIDES if a * b <= 2048]
    for i, (p0, q0) in enumerate(grid):
        fits = [s for s in PROJECT_IMAGES if s is None or (s[0] >= p0 and s[1] >= q0)]
        p, q = fits[i % len(fits)] or (p0, q0)
        cases.append((1 + 2 * (i % 2), p, q, p0, q0))
    for i, (p0, q0) in enumerate(PROJECT_NAMED):
        for n, s in ((3, None), (1, PROJECT_IMAGES[2 + i % 3])):
            c = (n,) + (s or (p0, q0)) + (p0, q0)
            if c not in cases:
                cases.append(c)
    return cases


FACTORS_N = [1, 15, 16, 17, 63, 64, 65, 129]
FACTORS_M = [1, 3, 4, 5, 625, 2047, 2048]
FACTORS_R = [1, 15, 16, 17, 63, 64, 65, 255, 256]


def factors_cases():
    """(n, m, r): every n at (625, 17) and (2048, 65); every m at n = 17 and 65; every r at (17, 625) and (129, 2048)"""
    cases = [(n, m, r) for n in FACTORS_N for m, r in ((625, 17), (2048, 65))]
    rs = {1: (1, 1), 3: (1, 1), 4: (1, 1), 5: (1, 1), 625: (255, 64), 2047: (256, 15), 2048: (256, 63)}
    cases += [(n, m, rs[m][i]) for m in FACTORS_M for i, n in enumerate((17, 65))]
    cases += [(n, m, r) for r in FACTORS_R for n, m in ((17, 625), (129, 2048))]
    return sorted(set(cases))


@functools.lru_cache(maxsize=8)
def gram_case(n, p, q, form, k=0, null_mean=False):
    """X, mean (or None), P (or None), the expected Gram"""
    X = int_stack(n, p, q, form)
    mean = None if null_mean else int_mean(p, q, form)
    Pm = int_proj(q if form == 1 else p, k, form) if form else None
    assert is_exact_gram(X, mean, form, Pm), (n, p, q, form, k)
    return X, mean, Pm, gram_ref(centred(X, mean), form, Pm)


@functools.lru_cache(maxsize=8)
def project_case(n, p, q, p0, q0):
    """X, mean, A, B, the expected U.  The projector seeds advance until every image's U has a non-zero in its last row
    a = p0 - 1 and in its last column b = q0 - 1 (a sum of a few small integers can cancel)"""
    X, mean = int_stack(n, p, q, 3), int_mean(p, q, 3)
    for seed in range(4, 40, 2):
        A, B = int_proj(p, p0, seed), int_proj(q, q0, seed + 1)
        U = project_ref(centred(X, mean), A, B)
        U3 = U.reshape(n, p0, q0)
        if np.all(np.any(U3[:, p0 - 1, :] != 0, axis=1)) and np.all(np.any(U3[:, :, q0 - 1] != 0, axis=1)):
            break
    assert is_exact_project(X, mean, A, B), (n, p, q, p0, q0)
    return X, mean, A, B, U


@functools.lru_cache(maxsize=8)
def factors_case(n, m, r):
    """U, G, the expected F"""
    rng = np.random.default_rng([n, m, r])
    U = rng.integers(-2, 3, (n, m)).astype(np.float32)
    U[n - 1, m - 1] = U[0, 0] = U[n - 1, 0] = U[0, m - 1] = 2.0
    G = int_proj(m, r, 6)
    assert is_exact_factors(U, G), (n, m, r)
    return U, G, factors_ref(U, G)


# ---- real-valued builders and bounds

def real_stack(n, p, q, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, p, q)) + 0.3 * rng.standard_normal((1, p, q)) + 1.0).astype(np.float32)


def real_proj(K, k, seed):
    """an orthonormal basis rounded to f32"""
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((K, k)))[0].astype(np.float32)


def f32_mean(X):
    return np.asarray(X, np.float64).mean(axis=0).astype(np.float32)


def gram_bound(Xc, form, Pm=None):
    """(N + 2 K + 8) u Wabs^T Wabs per entry (the module docstring)"""
    n, p, q = Xc.shape
    if form == 0:
        Wabs, K, k = np.abs(Xc).reshape(n * p, q), 0, p
    else:
        Wabs, K, k = w_stream(np.abs(Xc), form, np.abs(np.asarray(Pm, np.float64))), (q if form == 1 else p), Pm.shape[1]
    N = min(n, run_images(form, p)) * k
    return (N + 2 * K + 8) * U24 * (Wabs.T @ Wabs)


def project_bound(Xc, A, B):
    """(p + q + 8) u |A|^T |Xc| |B| per entry"""
    n, p, q = Xc.shape
    return (p + q + 8) * U24 * project_ref(np.abs(Xc), np.abs(A), np.abs(B))


def factors_bound(U, G):
    """(m + 8) u |U| |G| per entry"""
    return (U.shape[1] + 8) * U24 * factors_ref(np.abs(U), np.abs(G))


def mean_bound(X):
    """(n + 1) 2^-53 sum |x| / n + u |mean| per pixel"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    return (n + 1) * U53 * np.abs(X).sum(axis=0) / n + U24 * np.abs(X.mean(axis=0))


def chained_factors_bound(Xc, A, B, G):
    """F = f32(A^T Xc B) G from A, B, G: the device's U is within bU = project_bound of the float64 U, the recomputation rounds
    its own U to f32 (u |U|), both carried through |G|; the chain of m terms runs over the device's |U| <= |U| + bU"""
    U = project_ref(Xc, A, B)
    bU = project_bound(Xc, A, B)
    Ga = np.abs(np.asarray(G, np.float64))
    return (U.shape[1] + 8) * U24 * ((np.abs(U) + bU) @ Ga) + (bU + U24 * np.abs(U)) @ Ga


@functools.lru_cache(maxsize=None)
def real_gram_case(form):
    """X, the f32 mean (None for the second stage, form 3), P, the float64 Gram, the bound"""
    if form == 3:
        X, mean, Pm = real_stack(40, 1, 37, 13), None, None
    else:
        X = real_stack(5, 33, 47, 10 + form)
        mean, Pm = f32_mean(X), (real_proj(47 if form == 1 else 33, 5, 20 + form) if form else None)
    Xc = centred(X, mean)
    return X, mean, Pm, gram_ref(Xc, form % 3, Pm), gram_bound(Xc, form % 3, Pm)


@functools.lru_cache(maxsize=None)
def real_project_case():
    X = real_stack(3, 33, 47, 31)
    mean, A, B = f32_mean(X), real_proj(33, 5, 32), real_proj(47, 4, 33)
    Xc = centred(X, mean)
    return X, mean, A, B, project_ref(Xc, A, B), project_bound(Xc, A, B)


@functools.lru_cache(maxsize=None)
def real_factors_case():
    U = np.random.default_rng(41).standard_normal((17, 30)).astype(np.float32)
    G = real_proj(30, 5, 42)
    return U, G, factors_ref(U, G), factors_bound(U, G)


@functools.lru_cache(maxsize=None)
def real_mean_case():
    X = real_stack(70, 5, 7, 51)
    return X, np.asarray(X, np.float64).mean(axis=0), mean_bound(X)


def cut10(a):
    """float32 with the mantissa cut to 10 bits"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)
    return b.view(np.float32)


def f32_gram(X, mean, form, Pm, cut=lambda a: a):
    """the device's products in float32 numpy; cut is applied to every operand of every product"""
    n, p, q = X.shape
    Xc = cut(X - mean if mean is not None else X)
    if form == 0:
        Z = Xc.reshape(n * p, q)
    elif form == 1:
        Z = cut(np.matmul(Xc, cut(Pm)).transpose(0, 2, 1).reshape(-1, p))
    else:
        Z = cut(np.matmul(cut(Pm).T, Xc).reshape(-1, q))
    assert Z.dtype == np.float32
    return (Z.T @ Z).astype(np.float64)


def f32_project(X, mean, A, B, cut=lambda a: a):
    W1 = cut(np.matmul(cut(X - mean), cut(B)))
    U = np.matmul(cut(A).T, W1)
    assert U.dtype == np.float32
    return U.reshape(X.shape[0], -1).astype(np.float64)


# ---- the builders' own properties

def test_float64_products_of_integers_equal_int64():
    X, mean, Pm, ref = gram_case(33, 20, 24, 1, 5)
    Xi, Pi = (X - mean).astype(np.int64), Pm.astype(np.int64)
    Z = np.einsum("irc,cj->ijr", Xi, Pi).reshape(-1, 20)
    assert ref.dtype == np.float64 and np.array_equal(ref, (Z.T @ Z).astype(np.float64))
    X, mean, A, B, U = project_case(3, 33, 47, 17, 17)
    Xi = (X - mean).astype(np.int64)
    assert np.array_equal(U, np.einsum("ra,irc,cb->iab", A.astype(np.int64), Xi, B.astype(np.int64)).reshape(3, -1))
    Uf, G, F = factors_case(17, 625, 17)
    assert np.array_equal(F, Uf.astype(np.int64) @ G.astype(np.int64))


def test_case_lists_cover_the_issue():
    mc = mean_cases()
    for n in MEAN_N:
        assert len({(p, q) for nn, p, q in mc if nn == n}) >= 2
    for p, q in MEAN_PQ:
        assert len({n for n, pp, qq in mc if (pp, qq) == (p, q)}) >= 2
    assert sorted(p * q for p, q in MEAN_PQ) == [1, 63, 64, 65, 255, 256, 257] and any(p == 1 for p, q in MEAN_PQ)
    assert [d for n, p, d in GRAM0_TILE] == GRAM0_D and tile_geometry(129) == (2, 80) and tile_geometry(2048) == (16, 128)
    assert [-(-n // run_images(0, 33)) for n in (61, 62, 63)] == [1, 1, 2] and run_images(0, 33) * 33 % 16 == 14
    assert [-(-n // run_images(0, 256)) for n in (8, 9, 128, 129, 136, 137)] == [1, 2, 16, 17, 17, 18]
    assert {q for n, p, q in STAGE2} >= set(STAGE2_Q) and all(p == 1 for n, p, q in STAGE2)
    assert sum(1 for q in STAGE2_Q if {n for n, p, qq in STAGE2 if qq == q} >= set(STAGE2_N)) >= 2
    assert -(-(16 * 2048 + 1) // 2048) == 17
    assert sorted({k for k, L, d in GRAM12_KLD}) == GRAM12_K and all(L >= k for k, L, d in GRAM12_KLD)
    for k in GRAM12_K:
        assert len([c for c in GRAM12_KLD if c[0] == k]) >= 2 and any(L == k for kk, L, d in GRAM12_KLD if kk == k)
    for d in GRAM12_D:
        assert len({k for k, L, dd in GRAM12_KLD if dd == d}) >= 2
    assert {L for k, L, d in GRAM12_KLD} >= set(GRAM12_L)
    assert [-(-n // 32) for n in GRAM12_RUN_N] == [1, 1, 1, 2, 16, 17, 17, 18, 33]
    pc = project_cases()
    pairs = {(p0, q0) for n, p, q, p0, q0 in pc}
    assert pairs == {(a, b) for a in PROJECT_SIDES for b in PROJECT_SIDES if a * b <= 2048} | set(PROJECT_NAMED)
    assert {(p, q) for n, p, q, p0, q0 in pc} >= set(PROJECT_IMAGES[1:]) and {n for n, *_ in pc} == {1, 3}
    assert all(p0 <= min(p, 64) and q0 <= min(q, 64) and p0 * q0 <= 2048 for n, p, q, p0, q0 in pc)
    assert all((3, p0, q0, p0, q0) in pc for p0, q0 in PROJECT_NAMED)
    fc = factors_cases()
    assert all(r <= min(m, 256) for n, m, r in fc)
    for vals, pos in ((FACTORS_N, 0), (FACTORS_M, 1), (FACTORS_R, 2)):
        for v in vals:
            assert len({c[:pos] + c[pos + 1:] for c in fc if c[pos] == v}) >= 2, (pos, v)


def test_integer_builders():
    X, M = int_stack(5, 3, 17), int_mean(3, 17)
    assert X.dtype == np.float32 and np.abs(X).max() == 2 and np.abs(M).max() == 1 and len(np.unique(M)) == 3
    assert np.all(X[-1, -1, [0, -1]] != 0) and is_integer_f32(X, M)
    for K, k in ((1, 1), (5, 5), (17, 16), (256, 64), (2048, 256)):
        Pm = int_proj(K, k)
        assert set(np.unique(Pm)) <= {-1.0, 0.0, 1.0}
        assert np.any(Pm[0] != 0) and np.any(Pm[-1] != 0) and np.any(Pm[:, 0] != 0) and np.any(Pm[:, -1] != 0)
        assert Pm[0, 0] != 0 and Pm[-1, -1] != 0 and Pm[0, -1] != 0 and Pm[-1, 0] != 0
        assert np.abs(Pm).sum(axis=0).max() <= 6
    assert not is_integer_f32(np.array([0.5])) and not is_integer_f32(np.array([2.0 ** 24 + 1]))


def test_exactness_at_the_largest_shapes():
    """the worst accumulators of the domain stay below 2^24, and the check does reject what exceeds it"""
    X, mean, Pm = int_stack(32, 256, 256, 1), int_mean(256, 256, 1), int_proj(256, 64, 1)
    assert is_exact_gram(X, mean, 1, Pm) and is_exact_gram(X, mean, 2, Pm)
    W = np.abs(w_stream(centred(X, mean), 1, Pm))
    worst = float((W.T @ W).max())                              # 32 images = one run
    print("worst per-run partial at 32 x 256 x 256, k = 64: %.0f" % worst)
    assert worst < LIMIT
    assert is_exact_gram(int_stack(9, 256, 17), int_mean(256, 17), 0) and 2048 * 9 < LIMIT
    assert not is_exact_gram(1000.0 * int_stack(9, 256, 17), None, 0)
    assert not is_exact_gram(X[:2] + np.float32(0.5), mean, 1, Pm)
    assert not is_exact_factors(np.full((2, 2048), 2.0 ** 13, np.float32), np.ones((2048, 1), np.float32))


@pytest.mark.parametrize("n,p,q", mean_cases())
def test_mean_cases(n, p, q):
    X = int_stack(n, p, q, 7)
    m = mean_ref(X)
    assert m.dtype == np.float32 and m.shape == (p, q) and is_integer_f32(X)
    # sensitive to the last image of a run of 64 and the first of the next, and to the last image and the last pixel
    for i in sorted({n - 1, min(n, SDR_MEAN_RUN) - 1, SDR_MEAN_RUN if n > SDR_MEAN_RUN else 0, (n - 1) // 64 * 64}):
        Y = X.copy()
        Y[i] = 0
        assert not np.array_equal(mean_ref(Y), m), i


def removed(Xc, images=None, rows=None, cols=None):
    Y = Xc.copy()
    Y[images if images is not None else slice(None), rows if rows is not None else slice(None),
      cols if cols is not None else slice(None)] = 0
    return Y


@pytest.mark.parametrize("n,p,q", GRAM0_TILE + GRAM0_RUNS + [c for c in STAGE2 if c[0] * c[2] <= 2049 * 129])
def test_gram0_cases_are_exact_and_sensitive(n, p, q):
    null = p == 1
    X, mean, _, ref = gram_case(n, p, q, 0, 0, null)
    assert (mean is None) == null and ref.shape == (q, q) and np.array_equal(ref, ref.T) and np.array_equal(ref, np.rint(ref))
    Xc = centred(X, mean)
    run = run_images(0, p)
    cuts = [dict(cols=q - 1), dict(images=n - 1, rows=p - 1), dict(images=min(n, run) - 1), dict(images=min(n, run) - 1, rows=p - 1)]
    if n > run:
        cuts += [dict(images=run), dict(images=(n - 1) // run * run), dict(images=(n - 1) // run * run - 1, rows=p - 1)]
    for cut in cuts:
        assert not np.array_equal(gram_ref(removed(Xc, **cut), 0), ref), cut
    assert ref[q - 1, q - 1] > 0 and ref[0, q - 1] == ref[q - 1, 0]


def gram12_shapes():
    out = []
    for form in (1, 2):
        out += [(3, d, L, form, k, False) if form == 1 else (3, L, d, form, k, False) for k, L, d in GRAM12_KLD]
        out += [(n, 20, 24, form, 5, n in GRAM12_NULL_MEAN_N) for n in GRAM12_RUN_N]
        out += [(3, p, q, form, 5, False) for p, q in GRAM12_RECT]
    return out


@pytest.mark.parametrize("n,p,q,form,k,null", gram12_shapes())
def test_gram12_cases_are_exact_and_sensitive(n, p, q, form, k, null):
    X, mean, Pm, ref = gram_case(n, p, q, form, k, null)
    d, K = (p, q) if form == 1 else (q, p)
    assert Pm.shape == (K, k) and ref.shape == (d, d) and np.array_equal(ref, ref.T) and np.array_equal(ref, np.rint(ref))
    Xc = centred(X, mean)
    side = dict(rows=p - 1) if form == 1 else dict(cols=q - 1)
    cuts = [side, dict(images=n - 1), dict(images=min(n, 32) - 1)]
    if n > 32:
        cuts += [dict(images=32), dict(images=(n - 1) // 32 * 32), dict(images=(n - 1) // 32 * 32 - 1)]
    for cut in cuts:
        assert not np.array_equal(gram_ref(removed(Xc, **cut), form, Pm), ref), cut
    for r, c in ((K - 1, None), (None, k - 1)):
        Q = Pm.copy()
        Q[r if r is not None else slice(None), c if c is not None else slice(None)] = 0
        assert not np.array_equal(gram_ref(Xc, form, Q), ref), (r, c)
    # the contracted index K - 1 of the image matters too
    last = dict(cols=q - 1) if form == 1 else dict(rows=p - 1)
    assert not np.array_equal(gram_ref(removed(Xc, **last), form, Pm), ref)


@pytest.mark.parametrize("n,p,q,p0,q0", project_cases())
def test_project_cases_are_exact_and_sensitive(n, p, q, p0, q0):
    X, mean, A, B, U = project_case(n, p, q, p0, q0)
    assert U.shape == (n, p0 * q0) and np.array_equal(U, np.rint(U))
    Xc = centred(X, mean)
    U3 = U.reshape(n, p0, q0)
    for cut in (dict(rows=p - 1), dict(cols=q - 1), dict(images=n - 1)):
        assert not np.array_equal(project_ref(removed(Xc, **cut), A, B), U), cut
    for which, r, c in (("A", p - 1, None), ("A", None, p0 - 1), ("B", q - 1, None), ("B", None, q0 - 1)):
        A2, B2 = A.copy(), B.copy()
        (A2 if which == "A" else B2)[r if r is not None else slice(None), c if c is not None else slice(None)] = 0
        assert not np.array_equal(project_ref(Xc, A2, B2), U), (which, r, c)
    # the last row a = p0 - 1 and the last column b = q0 - 1 of the layout a q0 + b hold values
    assert np.any(U3[:, p0 - 1, :] != 0) and np.any(U3[:, :, q0 - 1] != 0)
    # image i's row depends on image i alone
    assert np.array_equal(project_ref(Xc[n - 1:], A, B)[0], U[n - 1])


@pytest.mark.parametrize("n,m,r", factors_cases())
def test_factors_cases_are_exact_and_sensitive(n, m, r):
    U, G, F = factors_case(n, m, r)
    assert F.shape == (n, r) and np.array_equal(F, np.rint(F))
    for rr, c in ((m - 1, None), (None, r - 1)):
        Q = G.copy()
        Q[rr if rr is not None else slice(None), c if c is not None else slice(None)] = 0
        assert not np.array_equal(factors_ref(U, Q), F), (rr, c)
    V = U.copy()
    V[n - 1] = 0
    assert not np.array_equal(factors_ref(V, G), F)
    V = U.copy()
    V[:, m - 1] = 0
    assert not np.array_equal(factors_ref(V, G), F)
    assert np.any(F[n - 1] != 0) and np.any(F[:, r - 1] != 0)


@pytest.mark.parametrize("n,q", [(2049, 2048), (2047, 2048)])
def test_large_second_stage_cases_are_exact(n, q):
    X, mean, _, ref = gram_case(n, 1, q, 0, 0, True)
    assert mean is None and np.array_equal(ref, ref.T) and ref[q - 1, q - 1] > 0 and ref.max() <= 4 * n


# ---- the bounds are neither too tight nor vacuous

def report(name, err, bound):
    ratio = float(np.max(err / bound))
    print("RATIO %s %.4f" % (name, ratio))
    return ratio


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_gram_bound_separates_float32_from_a_10_bit_mantissa(form):
    X, mean, Pm, ref, bound = real_gram_case(form)
    assert np.all(bound > 0) and bound.shape == ref.shape
    inside = report("float32 numpy gram form %d" % form, np.abs(f32_gram(X, mean, form % 3, Pm) - ref), bound)
    outside = report("10-bit gram form %d" % form, np.abs(f32_gram(X, mean, form % 3, Pm, cut10) - ref), bound)
    assert inside <= 1.0 < outside


def test_project_bound_separates_float32_from_a_10_bit_mantissa():
    X, mean, A, B, ref, bound = real_project_case()
    inside = report("float32 numpy project", np.abs(f32_project(X, mean, A, B) - ref), bound)
    outside = report("10-bit project", np.abs(f32_project(X, mean, A, B, cut10) - ref), bound)
    assert inside <= 1.0 < outside


def test_factors_bound_separates_float32_from_a_10_bit_mantissa():
    U, G, ref, bound = real_factors_case()
    inside = report("float32 numpy factors", np.abs((U @ G).astype(np.float64) - ref), bound)
    outside = report("10-bit factors", np.abs((cut10(U) @ cut10(G)).astype(np.float64) - ref), bound)
    assert inside <= 1.0 < outside


def test_mean_bound_separates_double_from_float32_sums():
    X, ref, bound = real_mean_case()
    exact = np.array([[np.float32(float(np.sum(X[:, r, c].astype(np.longdouble)) / X.shape[0])) for c in range(X.shape[2])]
                      for r in range(X.shape[1])])
    inside = report("double mean", np.abs(exact.astype(np.float64) - ref), bound)
    # a float32 running sum, and a mean whose result is cut to 10 bits, fall outside
    run32 = np.zeros(X.shape[1:], np.float32)
    for i in range(X.shape[0]):
        run32 = run32 + X[i]
    outside = report("float32 running-sum mean", np.abs((run32 / np.float32(X.shape[0])).astype(np.float64) - ref), bound)
    outside10 = report("10-bit mean", np.abs(cut10(exact).astype(np.float64) - ref), bound)
    assert inside <= 1.0 < min(outside, outside10)


def test_chained_bound_holds_for_float32_numpy():
    X, mean, A, B, ref, bound = real_project_case()
    G = real_proj(20, 5, 61)
    Xc = centred(X, mean)
    F = factors_ref(project_ref(Xc, A, B).astype(np.float32), G)
    cb = chained_factors_bound(Xc, A, B, G)
    got = (f32_project(X, mean, A, B).astype(np.float32) @ G).astype(np.float64)
    got10 = (cut10(f32_project(X, mean, A, B, cut10)) @ cut10(G)).astype(np.float64)
    assert report("float32 numpy chained factors", np.abs(got - F), cb) <= 1.0 < report("10-bit chained factors", np.abs(got10 - F), cb)
