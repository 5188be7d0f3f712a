"""-m gpu: the GSL form of the rank-deficient covariance on the device (lsqfit_amd/csrc/rankdef_dev.hip: blocked Cholesky
with diagonal pivoting and a rank exit, then the positive-definite chain on the kept block) -- the kernel on its own through
lsqamd_op_pivoted_inverse_dev against an extended-precision inverse of G[S, S], and through the fitters.

Null directions are put into J exactly: zero columns, 0.5 x a kept column, and HALF the sum of two kept columns (after either
addend is taken, a plain sum a + b and the other addend have the same residual: which of the two survives would hang on
rounding; half the sum always loses).  Their sources are the kept columns of below-median scale, so what is left of a dropped
column is rounding noise far below the floor n eps max G_ii, and every kept pivot is orders of magnitude above it -- checked on
every input with the host arithmetic (lsqamd_op_truncated_inverse) before anything goes to the GPU.
Bound: max |cov - ref| <= 16 n eps cond_2(G_SS) max |ref|, the standard bound of a Cholesky-based inverse."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import gpu_util as gu
from tests.test_gpu_eigh_blocks import amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
#        name: (n, dropped, extra ld, twins)
CASES = {'n5': (5, 2, 0, False), 'n64': (64, 3, 0, False), 'n65': (65, 4, 0, False), 'n65-ld': (65, 4, 15, False),
         'n65-twins': (65, 1, 0, True), 'n130-exit-in-first-panel': (130, 90, 0, False), 'n130-full-rank': (130, 0, 0, False),
         'n200-exit-mid-panel': (200, 50, 0, False), 'n200-exit-on-boundary': (200, 72, 0, False)}


def refined_inverse(G, cols=None):
    """columns `cols` (default: all) of inv(G): numpy's fp64 inverse, then Newton steps X <- X + X (I - G X) in np.longdouble"""
    n = G.shape[0]
    cols = np.arange(n) if cols is None else np.asarray(cols)
    X0 = np.linalg.inv(G).astype(np.longdouble)
    Gl, X, E = G.astype(np.longdouble), X0[:, cols].copy(), np.eye(n, dtype=np.longdouble)[:, cols]
    for _ in range(3):
        X = X + X0 @ (E - Gl @ X)
    return X


def bound_ratio(cov, keep, ref, G):
    Gs = G[np.ix_(keep, keep)]
    return float(np.max(np.abs(cov[np.ix_(keep, keep)] - ref)) / (16 * len(G) * EPS * np.linalg.cond(Gs) * np.max(np.abs(ref))))


@functools.lru_cache(maxsize=None)
def case(name):
    """G = J^T J (read-only), the kept set, the reference on it, the host op's ratio to the bound"""
    n, dropped, _, twins = CASES[name]
    rng = np.random.default_rng(1000 + n + dropped)
    order = rng.permutation(n)
    keep, dep = np.sort(order[dropped:]), np.sort(order[:dropped])
    scale = 10.0 ** rng.uniform(-1.5, 1.5, n)
    J = np.zeros((2 * n, n))
    J[:, keep] = rng.standard_normal((2 * n, keep.size)) * scale[keep]
    if twins:                       # the largest column twice: the tie is met at the first pivot, the lower index is kept
        lo, hi = sorted((int(keep[0]), int(dep[0])))
        J[:, lo] = 100.0 * rng.standard_normal(2 * n)
        J[:, hi] = J[:, lo]
        keep, dep = np.sort(np.append(np.setdiff1d(keep, [lo, hi]), lo)), np.array([hi])
    else:
        small = keep[scale[keep] <= np.median(scale[keep])]
        for t, c in enumerate(dep):
            a, b = small[(5 * t) % small.size], small[(5 * t + 2) % small.size]
            J[:, c] = (0.0, 0.5 * J[:, a], 0.5 * (J[:, a] + J[:, b]))[t % 3]
    G = J.T @ J
    from lsqfit_amd import _lib
    host, k = np.empty((n, n)), C.c_int32(-1)
    assert _lib.load().lsqamd_op_truncated_inverse(_lib.dptr(G), n, 2 * n, 0, _lib.dptr(host), C.byref(k)) == 0
    assert k.value == dropped and np.array_equal(np.flatnonzero(~host.any(axis=1)), dep), name   # the condition on the input
    ref = np.asarray(refined_inverse(G[np.ix_(keep, keep)]), float)
    G.setflags(write=False)
    return G, keep, dep, ref, bound_ratio(host, keep, ref, G)


def run_op(G, ld):
    import torch
    from lsqfit_amd import _lib
    lib, n = _lib.load(), G.shape[0]
    dG = torch.full((n, ld), float('nan'), dtype=torch.float64, device='cuda')
    dG[:, :n] = torch.from_numpy(np.array(G))
    cov = torch.full((n, n + 3), float('nan'), dtype=torch.float64, device='cuda')
    perm = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    rank = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    wb = lib.lsqamd_op_pivoted_inverse_dev_work_bytes(n)
    work = torch.empty(wb // 8 + 1, dtype=torch.float64, device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.lsqamd_op_pivoted_inverse_dev(None, ptr(dG), n, ld, ptr(cov), n + 3, ptr(perm), ptr(rank), ptr(work), wb) == 0
    torch.cuda.synchronize()
    return cov.cpu().numpy()[:, :n], perm.cpu().numpy(), rank.cpu().numpy()


@pytest.mark.parametrize('name', list(CASES))
def test_pivoted_inverse_against_extended_precision(amd, name):
    G, keep, dep, ref, host_ratio = case(name)
    n = G.shape[0]
    cov, perm, rank = run_op(G, n + CASES[name][2])
    assert rank[1] == 0 and rank[0] == keep.size and sorted(perm) == list(range(n))
    assert np.array_equal(np.sort(perm[:rank[0]]), keep)
    assert not cov[dep].any() and not cov[:, dep].any()
    assert np.array_equal(cov, cov.T)
    ratio = bound_ratio(cov, keep, ref, G)
    print('rankdef %-26s n %3d rank %3d  error / bound: device %.3e  host %.3e' % (name, n, rank[0], ratio, host_ratio))
    assert ratio <= 1.0


def test_nonfinite_diagonal_is_a_status(amd):
    G = np.array(case('n65')[0])
    G[40, 40] = np.inf
    assert run_op(G, 65)[2][1] == 1


def small_fit(amd, kind, solver):
    """12 rows, 4 parameters, linear: the column of p2 is zero ('dead'), or the column of p3 repeats that of p1 ('twins')"""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((12, 4)) * np.array([3.0, 1.0, 0.3, 1.0])
    X[:, 2 if kind == 'dead' else 3] = 0.0 if kind == 'dead' else X[:, 1]
    model = amd.expr(' + '.join('s%d*p%d' % (i, i) for i in range(4)), ['p%d' % i for i in range(4)], xnames=('s0', 's1', 's2', 's3'))
    pr = amd.DeviceProblem(model, X, amd.Whitening(X @ np.array([1.0, -2.0, 0.5, 0.25]), np.ones(12)))
    ans = amd.mi355x_lm(np.zeros(4), 12, None, tol=(1e-10, 0.0, 0.0), solver=solver, problem=pr)
    pr.close()
    return X, ans


@pytest.mark.parametrize('kind,solver', [('dead', 'cholesky'), ('twins', 'cholesky'), ('dead', 'qr')])
def test_small_fits_device_route_equals_host_route(amd, monkeypatch, kind, solver):
    monkeypatch.setenv('LSQAMD_RANKDEF', 'host')
    X, host = small_fit(amd, kind, solver)
    monkeypatch.setenv('LSQAMD_RANKDEF', 'device')
    X, dev = small_fit(amd, kind, solver)
    keep = np.flatnonzero(host.cov.any(axis=1))
    assert host.error is None and dev.error is None and dev.cov_dropped == host.cov_dropped == 1
    assert list(keep) == ([0, 1, 3] if kind == 'dead' else [0, 1, 2])
    assert np.array_equal(np.flatnonzero(dev.cov.any(axis=1)), keep) and np.array_equal(dev.cov, dev.cov.T)
    assert bound_ratio(dev.cov, keep, host.cov[np.ix_(keep, keep)], X.T @ X) <= 1.0
    assert dev.logdet_jtj == -np.inf


def test_fit_above_the_host_cap_gets_its_covariance(amd):
    """No knob, P = 2050 > LSQAMD_RANKDEF_MAXP's default, no prior, noisy data, start at the truth.  Two frequencies are
    zero: d/dw of a cos(w x) is -a x sin(0), an exactly zero column wherever the amplitudes go, and the two amplitudes share
    the column cos(0) = 1 -- three directions the data do not see, of which the twin amplitudes leave it to the pivot order
    which of them is kept.  (The parent commit reports "covariance undefined" here.)  The reference is refined on seventeen
    whole columns of the kept block -- all rows of each, the dropped parameters' neighbours among them: an extended-
    precision product for all 2047 columns would take minutes."""
    K, N, dead = 1025, 4096, np.array([300, 777])
    x = np.arange(N, dtype=float)
    p = np.concatenate([1.0 + 0.5 * np.cos(np.arange(K)), np.pi * (np.arange(K) + 0.5) / 1100.0])
    p[K + dead] = 0.0
    y = gu.cosmix_fcn(x, p) + 1e-3 * np.random.default_rng(2050).standard_normal(N)
    fit = amd.nonlinear_fit(data=(x, y, np.ones(N)), model=amd.cosmix(K), p0=p, tol=1e-6, maxit=30)
    assert fit.error is None and fit.fitter_results.cov_dropped == 3
    dep = np.flatnonzero(~fit.cov.any(axis=1))
    keep = np.setdiff1d(np.arange(2 * K), dep)
    assert dep.size == 3 and dep[0] in dead and list(dep[1:]) == list(K + dead)
    assert not fit.cov[:, dep].any() and np.array_equal(fit.cov, fit.cov.T)
    J = gu.cosmix_jac(x, fit.pmean)
    Gs = (J.T @ J)[np.ix_(keep, keep)]
    cols = np.unique(np.r_[0, K - 1, K, 2 * K - 4, np.searchsorted(keep, dep), np.searchsorted(keep, dep) - 1, 5:2040:255])
    ref = np.asarray(refined_inverse(Gs, cols), float)
    err = np.max(np.abs(fit.cov[np.ix_(keep, keep)][:, cols] - ref))
    ratio = err / (16 * 2 * K * EPS * np.linalg.cond(Gs) * np.max(np.abs(ref)))
    print('rankdef fit P = 2050: error / bound %.3e' % ratio)
    assert ratio <= 1.0
