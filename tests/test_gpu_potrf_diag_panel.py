"""potrf_upper with the next diagonal block updated in the row-panel launch (the default) against the path that
updates it in workgroup 0 of the fused launch (LSQAMD_DIAG_IN_PANEL=0, read per call): the two must agree byte
for byte, positive definite or not.

A step takes the new path when it ends in a fused launch of at most 240 trailing tiles (every one at these sizes)
and the step before it ended in a fused launch too: with the fuse threshold of 10 trailing tiles, n = 640 has one
fused step (the first: the new path never runs, the knob must change nothing), n = 768 has two (one on the new
path), n = 1152 has five (four on the new path) and an unfused tail."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOB = 'LSQAMD_DIAG_IN_PANEL'
SIZES = [(640, 768), (768, 896), (1152, 1152)]       # (n, n_cols): with and without the pad column block


@pytest.fixture(scope='module')
def env():
    import torch
    from lsqfit_amd import _lib
    lib = _lib.load()
    return torch, lib


_SPD = {}


def spd(n):
    """(A, b) as tests/test_gpu_ops.py::test_potrf_upper_tile_aligned_fused_path builds them; made once per size"""
    if n not in _SPD:
        rng = np.random.default_rng(n)
        G = rng.standard_normal((n + 64, n))
        A = G.T @ G + 0.1 * np.eye(n)
        A.setflags(write=False)
        b = rng.standard_normal(n)
        b.setflags(write=False)
        _SPD[n] = (A, b)
    return _SPD[n]


def new_path_steps(n):
    fused = [k for k in range(n // 128) if (lambda m: m > 0 and m * (m + 1) // 2 >= 10)(n // 128 - k - 1)]
    return max(len(fused) - 1, 0)


def factor(env, A, b, n, n_cols, lda, knob):
    """-> (A after the call, work, info) as device tensors; knob None = the default path"""
    torch, lib = env
    Ab = np.zeros((n, lda))
    Ab[:, :n] = np.triu(A)
    if n_cols > n:
        Ab[:, n] = b
    dA = torch.from_numpy(Ab).cuda()
    wbytes = lib.lsqamd_op_potrf_work_bytes(n)
    work = torch.full((wbytes // 8 + 8,), float('nan'), dtype=torch.float64, device='cuda')
    info = torch.zeros(4, dtype=torch.int32, device='cuda')
    saved = os.environ.pop(KNOB, None)
    try:
        if knob is not None:
            os.environ[KNOB] = knob
        rc = lib.lsqamd_op_potrf_upper(None, dA.data_ptr(), n, lda, n_cols, work.data_ptr(), wbytes, info.data_ptr())
        torch.cuda.synchronize()
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved
    assert rc == 0
    return dA, work, info


def assert_same_bytes(torch, n, old, new):
    (Ao, wo, io), (An, wn, inn) = old, new
    upper = torch.triu(torch.ones(Ao.shape, dtype=torch.bool, device='cuda'))   # column >= row: pad columns included
    assert torch.equal(Ao.view(torch.int64)[upper], An.view(torch.int64)[upper])
    nold = (n // 128) * 128 * 128                                               # the inverses: the old work size
    assert torch.equal(wo.view(torch.int64)[:nold], wn.view(torch.int64)[:nold])
    assert torch.equal(io, inn)


@pytest.mark.parametrize('pad_lda', [False, True])
@pytest.mark.parametrize('n,n_cols', SIZES)
def test_same_bytes_as_fused_workgroup_update(env, n, n_cols, pad_lda):
    torch, _ = env
    A, b = spd(n)
    lda = n + 136 if pad_lda else n_cols
    old = factor(env, A, b, n, n_cols, lda, '0')
    new = factor(env, A, b, n, n_cols, lda, None)
    assert int(new[2][0]) == 0
    assert_same_bytes(torch, n, old, new)
    # the scratch tile behind the inverses is written on the new path only: the knob really selects the path
    nold = (n // 128) * 128 * 128
    assert bool(torch.isnan(old[1][nold:nold + 128 * 128]).all())
    wrote = bool(torch.isfinite(new[1][nold:nold + 128 * 128]).all())
    assert wrote == (new_path_steps(n) > 0)
    assert bool(torch.isnan(new[1][nold + 128 * 128:]).all())                   # nothing past the declared size


def test_same_bytes_across_the_tile_limit(env):
    """n = 3072: 276 and 253 trailing tiles at steps 0 and 1 (workgroup 0 updates), 231 at step 2, the first on the new
    path -- the scratch tile it reads was left by a fused launch that itself took the old path."""
    torch, _ = env
    n = 3072
    rng = np.random.default_rng(n)
    R = rng.standard_normal((n, n))
    A = R + R.T + 4.0 * np.sqrt(n) * np.eye(n)      # symmetric, spectrum of R + R^T within +- 2 sqrt(2 n): positive definite
    b = rng.standard_normal(n)
    old = factor(env, A, b, n, n + 128, n + 128, '0')
    new = factor(env, A, b, n, n + 128, n + 128, None)
    assert int(new[2][0]) == 0
    assert_same_bytes(torch, n, old, new)
    U = np.triu(new[0].cpu().numpy()[:, :n])
    assert np.abs(U.T @ U - A).max() < 1e-11 * np.abs(A).max()


@pytest.mark.parametrize('pad_lda', [False, True])
@pytest.mark.parametrize('n,n_cols', SIZES)
def test_against_numpy(env, n, n_cols, pad_lda):
    torch, _ = env
    A, b = spd(n)
    lda = n + 136 if pad_lda else n_cols
    dA, work, info = factor(env, A, b, n, n_cols, lda, None)
    assert int(info[0]) == 0
    out = dA.cpu().numpy()
    Uref = np.linalg.cholesky(A).T
    scale = np.abs(Uref).max()
    assert np.abs(np.triu(out[:, :n]) - Uref).max() < 1e-11 * scale             # the existing fused-path test's bound
    if n_cols > n:
        assert np.abs(out[:, n] - np.linalg.solve(Uref.T, b)).max() < 1e-10 * np.abs(b).max()


@pytest.mark.parametrize('n,n_cols,row', [(640, 768, 200),      # second block
                                          (768, 896, 300),      # the one block of n = 768 the new workgroups update
                                          (1152, 1152, 700)])   # the block of the last fused launch
def test_not_positive_definite(env, n, n_cols, row):
    torch, _ = env
    A, b = spd(n)
    A = A.copy()
    A[row, row] = -1.0            # leading minors up to `row` stay positive definite: pivot `row` is the first to fail
    old = factor(env, A, b, n, n_cols, n_cols, '0')
    new = factor(env, A, b, n, n_cols, n_cols, None)
    assert int(new[2][0]) == row + 1
    assert_same_bytes(torch, n, old, new)
