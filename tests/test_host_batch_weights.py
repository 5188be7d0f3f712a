"""Host side of per-fit data covariances in the batched engine: ``whiten.stack_whitenings`` against one ``Whitening`` per fit
(bit for bit), its refusals, and the ``BatchedFits`` argument checks that need no device."""
import numpy as np
import pytest

from lsqfit_amd.whiten import BatchWhitening, Whitening, stack_whitenings


def spd(rng, n, scale):
    """well conditioned: correlation matrix 0.8 I + 0.2 (positive correlations), eigenvalues in [0.8, 0.8 + 0.2 n]"""
    U = rng.uniform(0.1, 0.9, (n, 2 * n))
    c = U @ U.T
    d = 1.0 / np.sqrt(np.diag(c))
    c = 0.8 * np.eye(n) + 0.2 * c * np.outer(d, d)
    return c * np.outer(scale, scale)


def layout(rng, N, blocks, B):
    """B error specs dict(sdev=, blocks=) with the same (row0, size) list and per-fit values"""
    out = []
    for b in range(B):
        sd = rng.uniform(0.5, 2.0, N) * (0.5 + b)
        out.append(dict(sdev=sd, blocks=[(r0, spd(rng, n, sd[r0:r0 + n])) for r0, n in blocks]))
    return out


def test_stack_equals_one_whitening_per_fit():
    rng = np.random.default_rng(1)
    N, blocks, B = 60, [(0, 9), (12, 5), (30, 17)], 4
    errs = layout(rng, N, blocks, B)
    ym = rng.standard_normal((B, N))
    bw = stack_whitenings(ym, errs, svdcut=1e-12, engine='host')
    assert isinstance(bw, BatchWhitening) and bw.n_fits == B and bw.n_data == N and bw.perm is None
    assert bw.wdiag.shape == (B, N) and bw.wt.shape == (B, 9 * 9 + 5 * 5 + 17 * 17)
    assert list(bw.row0) == [0, 12, 30] and list(bw.size) == [9, 5, 17]
    for b in range(B):
        wh = Whitening(ym[b], errs[b], svdcut=1e-12, engine='host')
        row0, size, modes, tri, wt = wh.block_arrays()
        assert np.array_equal(bw.wdiag[b], wh.wdiag)
        assert np.array_equal(bw.wt[b], wt)
        assert bw.logdet_data[b] == wh.logdet_data
        assert np.array_equal(bw.modes, modes) and np.array_equal(bw.row0, row0) and np.array_equal(bw.size, size)
        assert bw.nchiv_data == wh.nchiv_data
    r0, s0, m0, t0, w0 = bw.block_arrays()
    assert np.array_equal(w0, bw.wt[0]) and np.array_equal(t0, bw.tri)


def test_stack_sdev_vectors_and_dense_matrices():
    """sdev vectors (no blocks) and dense covariance matrices whose components interleave (a shared row permutation)"""
    rng = np.random.default_rng(2)
    N, B = 11, 3
    sds = [rng.uniform(0.5, 2.0, N) for _ in range(B)]
    bw = stack_whitenings(np.zeros(N), sds, engine='host')
    assert bw.wt.shape == (B, 0) and len(bw.size) == 0 and bw.nchiv_data == N
    for b in range(B):
        wh = Whitening(np.zeros(N), sds[b], engine='host')
        assert np.array_equal(bw.wdiag[b], wh.wdiag) and bw.logdet_data[b] == wh.logdet_data
    covs = []
    for b in range(B):
        c = np.diag(sds[b] ** 2)
        c[0, 5] = c[5, 0] = 0.3 * sds[b][0] * sds[b][5]      # rows 0 and 5 correlated, 1-4 not: interleaved components
        covs.append(c)
    bw = stack_whitenings(np.zeros(N), covs, engine='host')
    wh0 = Whitening(np.zeros(N), covs[0], engine='host')
    assert bw.perm is not None and np.array_equal(bw.perm, wh0.perm)
    for b in range(B):
        wh = Whitening(np.zeros(N), covs[b], engine='host')
        assert np.array_equal(bw.wdiag[b], wh.wdiag) and bw.logdet_data[b] == wh.logdet_data
        assert np.array_equal(bw.wt[b], wh.block_arrays()[4])


def near_singular(rng, n, sd):
    """covariance with two nearly equal rows: its correlation matrix has an eigenvalue ~1e-6 of the largest"""
    c = spd(rng, n, np.ones(n))
    L = np.linalg.cholesky(c)
    L[1] = L[0] + 1e-3 * L[1]
    c = L @ L.T
    d = 1.0 / np.sqrt(np.diag(c))
    return c * np.outer(d, d) * np.outer(sd, sd)


def test_tri_is_the_and_over_fits():
    rng = np.random.default_rng(3)
    N, B = 40, 3
    errs = layout(rng, N, [(0, 8), (10, 17)], B)
    errs[1]['blocks'][1] = (10, near_singular(rng, 17, errs[1]['sdev'][10:27]))
    bw = stack_whitenings(np.zeros(N), errs, svdcut=1e-2, engine='host')
    whs = [Whitening(np.zeros(N), e, svdcut=1e-2, engine='host') for e in errs]
    tris = np.array([wh.block_arrays()[3] for wh in whs])
    assert list(tris[:, 1]) == [1, 0, 1]                       # the floor binds in fit 1's second block only
    assert np.array_equal(bw.tri, tris.min(axis=0)) and list(bw.tri) == [1, 0]
    for b in range(B):
        assert np.array_equal(bw.wt[b], whs[b].block_arrays()[4]) and bw.logdet_data[b] == whs[b].logdet_data


def test_other_block_structure_names_the_fit():
    rng = np.random.default_rng(4)
    N = 30
    errs = layout(rng, N, [(0, 6), (10, 7)], 3)
    errs[1] = layout(rng, N, [(0, 6), (11, 7)], 1)[0]
    with pytest.raises(ValueError, match='fit 1'):
        stack_whitenings(np.zeros(N), errs, engine='host')
    errs[1] = layout(rng, N, [(0, 6)], 1)[0]
    with pytest.raises(ValueError, match='fit 1'):
        stack_whitenings(np.zeros(N), errs, engine='host')
    with pytest.raises(ValueError, match='fit 2'):
        stack_whitenings(np.zeros(N), [np.ones(N), np.ones(N), np.ones(N - 1)], engine='host')


def test_other_modes_names_the_fit():
    """a negative svdcut DROPS the modes under the cut: fit 1's near-singular block keeps fewer than fit 0's"""
    rng = np.random.default_rng(5)
    N = 30
    errs = layout(rng, N, [(2, 12)], 3)
    errs[1]['blocks'][0] = (2, near_singular(rng, 12, errs[1]['sdev'][2:14]))
    m0 = Whitening(np.zeros(N), errs[0], svdcut=-1e-3, engine='host').block_arrays()[2]
    m1 = Whitening(np.zeros(N), errs[1], svdcut=-1e-3, engine='host').block_arrays()[2]
    assert m1[0] < m0[0] == 12
    with pytest.raises(ValueError, match='fit 1.*modes'):
        stack_whitenings(np.zeros(N), errs, svdcut=-1e-3, engine='host')


def test_batched_fits_argument_checks():
    from lsqfit_amd import BatchedFits, models
    model = models.cosmix(2)
    N = 12
    x, y = np.linspace(0, 1, N), np.zeros(N)
    pm, ps = np.zeros((3, 4)), np.ones((3, 4))
    errs = [np.ones(N)] * 3
    with pytest.raises(ValueError, match='not both'):
        BatchedFits(model, x, y, None, pm, ps, per_fit_yerr=errs, whitening=Whitening(y, np.ones(N), engine='host'))
    with pytest.raises(ValueError, match='2 entries.*3'):
        BatchedFits(model, x, y, None, pm, ps, per_fit_yerr=errs[:2])
    with pytest.raises(ValueError, match='2 entries.*3'):
        BatchedFits(model, x, y, None, pm, ps, whitening=errs[:2])           # (a list there: per-fit errors)
    with pytest.raises(ValueError, match='n_fits'):
        BatchedFits(model, x, y, None, None, None, per_fit_yerr=errs, n_fits=4)
    with pytest.raises(ValueError, match='rows'):
        BatchedFits(model, x, np.zeros((2, N)), None, None, None, per_fit_yerr=errs)
    with pytest.raises(ValueError, match='n_fits entries'):
        BatchedFits(model, x, y, None, pm, ps, per_fit_yerr=[])
