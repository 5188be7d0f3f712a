"""-m gpu: the two-sided Jacobi pivot solver (csrc/eigh_twosided.hip) on its own through lsqamd_op_eigh_pivots, and the
block-Jacobi route of csrc/eigh_large.hip that uses it, at a size the one-sided inner solve could not serve.

Against numpy.linalg.eigh, defects evaluated in numpy.longdouble; the bound is C_SOLVER = 8 times max(B eps lambda_max,
LAPACK's own defect), the constant test_gpu_eigh_blocks argues for.  Worst measured ratios: profiles/eigh_pivots.txt."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_eigh_blocks import EPS, amd, cluster, corr, gap, rankdef  # noqa: F401 (amd: fixture)

pytestmark = pytest.mark.gpu
C_SOLVER = 8.0


def defects(A, lam, V, tag, LD=np.longdouble):
    """(eigenvalues, residual, orthogonality) of (lam, V) over max(unit, LAPACK's own); printed, then held to C_SOLVER.
    (LD: numpy's extended-precision products are seconds at 1024 rows; the route tests evaluate in double, as
    test_gpu_eigh_large does)"""
    B = len(A)
    w, v = np.linalg.eigh(A)
    Al, eye = A.astype(LD), np.eye(B, dtype=LD)

    def two(l, X):
        X, l = X.astype(LD), l.astype(LD)
        return float(np.max(np.abs(Al @ X - X * l))), float(np.max(np.abs(X.T @ X - eye)))
    got, ref = (float(np.max(np.abs(lam - w))),) + two(lam, V), (0.0,) + two(w, v)
    unit = B * EPS * np.max(np.abs(w))
    print(tag, 'defect / max(unit, LAPACK):', ['%.3f' % (g / max(unit, r)) if max(unit, r) > 0 else g for g, r in zip(got, ref)])
    assert np.all(np.diff(lam) >= 0)
    for g, r in zip(got, ref):                                       # (the zero matrix: unit = 0, an exact result is demanded)
        assert g <= C_SOLVER * max(unit, r), (tag, got, ref, unit)


@pytest.mark.parametrize('B', [2, 3, 33, 63, 64])
def test_pivot_solver_against_lapack(amd, B):
    import torch
    from lsqfit_amd import _lib
    rng = np.random.default_rng(4000 + B)
    Q, _ = np.linalg.qr(rng.standard_normal((B, B)))
    l = rng.uniform(0.1, 1.0, (B + 1) // 2)
    paired = (Q * np.stack([l, -l], 1).ravel()[:B]) @ Q.T            # eigenvalues +l, -l: degenerate in A^2
    mats = [corr(rankdef(rng, B)), corr(gap(rng, B)), corr(cluster(rng, B)), (paired + paired.T) / 2, np.zeros((B, B))]
    if B >= 3:                                                       # what eigh_large's padding looks like
        bordered = np.zeros((B, B))
        d = B // 2
        keep = np.arange(B) != d
        bordered[np.ix_(keep, keep)] = corr(rankdef(rng, B - 1))
        bordered[d, d] = -1.0
        mats.append(bordered)
    nb, lda = len(mats), B + 3
    stride = lda * B + 5
    host = np.full(nb * stride, np.nan)
    for b, A in enumerate(mats):
        host[b * stride:b * stride + lda * B].reshape(B, lda)[:, :B] = A
    dA = torch.from_numpy(host).cuda()
    lam = torch.empty((nb, B), dtype=torch.float64, device='cuda')
    sweeps, status = (torch.full((nb,), -1, dtype=torch.int32, device='cuda') for _ in range(2))
    rc = _lib.load().lsqamd_op_eigh_pivots(None, B, nb, C.c_void_p(dA.data_ptr()), lda, stride, C.c_void_p(lam.data_ptr()),
                                           C.c_void_p(sweeps.data_ptr()), C.c_void_p(status.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    out, lam, sweeps, status = dA.cpu().numpy(), lam.cpu().numpy(), sweeps.cpu().numpy(), status.cpu().numpy()
    print('B=%d sweeps' % B, sweeps.tolist())
    assert np.all(status == 0) and np.all((1 <= sweeps) & (sweeps < 30))
    vecs = [out[b * stride:b * stride + lda * B].reshape(B, lda)[:, :B] for b in range(nb)]
    for b, A in enumerate(mats):
        defects(A, lam[b], vecs[b], 'B=%d matrix %d' % (B, b))
    if B >= 3:
        Vb, lb = vecs[5], lam[5]                                     # the bordered matrix
        j = np.flatnonzero(Vb[d] != 0.0)
        assert len(j) == 1 and lb[j[0]] == -1.0
        assert Vb[d, j[0]] == 1.0 and np.all(np.delete(Vb[:, j[0]], d) == 0.0)


def route(monkeypatch, B, inner=None):
    from lsqfit_amd.whiten import _Block, _device_regulate_eig
    monkeypatch.setenv('LSQAMD_EIGH_LARGE', 'device')
    if inner:
        monkeypatch.setenv('LSQAMD_EIGH_LARGE_INNER', inner)
    A = corr(rankdef(np.random.default_rng(1000 + B), B))
    k = _device_regulate_eig([A], 1e-3, False)[0]
    assert k is not None and k['sweeps'] < 30
    print('B=%d sweeps=%d' % (B, k['sweeps']))
    defects(A, _Block._to_host(k['lam_dev']), _Block._to_host(k['vec_dev']), 'B=%d inner=%s' % (B, inner), np.float64)


def test_singular_block_of_1024_rows_comes_back(amd, monkeypatch):
    route(monkeypatch, 1024)


def test_onesided_inner_solve_stays_reachable(amd, monkeypatch):
    route(monkeypatch, 320, 'onesided')
