"""-m gpu: the eigen-mode route of the whitening set-up on the device (lsqamd_whiten_blocks_eig: batched
Jacobi eigensolver csrc/eigh_blocks.hip + the weights kernel in csrc/whiten.hip) for the blocks the svdcut
floor binds -- against LAPACK, against the host engine, and through whole fits.

Measured on an MI355X (profiles/eigh_blocks.txt): the solver's defects are at most 1.05 x the bound's unit
B eps lambda_max (B = 256, orthogonality of the two-level spectrum); C_SOLVER = 8 is that with room for other
seeds and rounding orders, inside the limit of 16 the tridiagonal-against-Jacobi argument allows.

Routing: fewer than whiten.EIGH_DEVICE_MIN_BLOCKS handed-back blocks of one size stay on the host (measured
crossover), so the whitening test runs batches of that many; the fit-sized tests force the device route with
the LSQAMD_EIGH=device knob."""
import functools

import numpy as np
import pytest

from tests import gpu_util as gu

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
C_SOLVER = 8.0


@pytest.fixture(scope='module')
def amd():
    import lsqfit_amd
    from lsqfit_amd import _lib
    _lib.load()
    return lsqfit_amd


def rankdef(rng, B):
    """sample covariance of B // 2 Gaussian samples with random scales: exactly singular"""
    X = rng.standard_normal((max(B // 2, 2), B)) * rng.uniform(0.1, 10.0, B)
    return np.cov(X, rowvar=False)


def spectrum(rng, B, lam):
    Q, _ = np.linalg.qr(rng.standard_normal((B, B)))
    C = (Q * lam) @ Q.T
    s = rng.uniform(0.1, 10.0, B)
    return (C + C.T) / 2 * np.outer(s, s)


def gap(rng, B, cut=1e-3):
    """two levels, a factor 100 on either side of the cut"""
    return spectrum(rng, B, np.where(np.arange(B) < (B + 1) // 2, 1.0, abs(cut) / 100))


def cluster(rng, B):
    """eigenvalues repeated in groups of four"""
    return spectrum(rng, B, np.geomspace(1.0, 1e-3, (B + 3) // 4).repeat(4)[:B])


def corr(c):
    sd = np.sqrt(np.diag(c))
    a = c / np.outer(sd, sd)
    a[np.diag_indices_from(a)] = 1.0
    return a


def clear_of_floor(c, cut):
    """no eigenvalue of the correlation matrix within a factor 10 of the floor: nmod is unambiguous"""
    w = np.linalg.eigvalsh(corr(c))
    r = w / (abs(cut) * w[-1])
    return not np.any((r > 0.1) & (r < 10.0))


@functools.lru_cache(maxsize=None)
def whitening_inputs(B, n=32):
    """n rankdef and n gap blocks (read-only: shared by the cases of one size; the gap kind depends on |cut| = 1e-3 only)"""
    rng = np.random.default_rng(7000 + B)
    covs = []
    for f in (rankdef, gap):
        draws = [f(rng, B) for _ in range(3 * n)]                    # (a few draws put an eigenvalue near the floor: passed over)
        covs += [c for c in draws if clear_of_floor(c, 1e-3)][:n]
    assert len(covs) == 2 * n and all(clear_of_floor(c, 1e-3) for c in covs)
    return covs


@pytest.mark.parametrize('B', [2, 3, 17, 64, 65, 128, 129, 200, 256])
def test_solver_against_lapack(amd, B):
    from lsqfit_amd.whiten import _Block, _device_regulate_eig
    rng = np.random.default_rng(1000 + B)
    mats = [corr(f(rng, B)) for f in (rankdef, gap, cluster)]        # unit diagonal: the device's correlation matrix IS this
    out = _device_regulate_eig(mats, 1e-3, False)                    # (floor form: every mode kept, so every block comes back)
    for A, k in zip(mats, out):
        assert k is not None and 1 <= k['sweeps'] < 30
        lam, V = _Block._to_host(k['lam_dev']), _Block._to_host(k['vec_dev'])
        w, v = np.linalg.eigh(A)
        unit = B * EPS * w[-1]
        eye = np.eye(B)
        got = (np.max(np.abs(lam - w)), np.max(np.abs(A @ V - V * lam)), np.max(np.abs(V.T @ V - eye)))
        ref = (0.0, np.max(np.abs(A @ v - v * w)), np.max(np.abs(v.T @ v - eye)))
        assert np.all(np.diff(lam) >= 0)
        for g, r in zip(got, ref):
            assert g <= C_SOLVER * max(unit, r)


@pytest.mark.parametrize('cut', [1e-3, -1e-3])
@pytest.mark.parametrize('B', [5, 64, 129, 256])
def test_whitening_against_host_engine(amd, B, cut):
    from lsqfit_amd.whiten import regulate_blocks
    covs = whitening_inputs(B)                                       # 64 blocks: inside the device route's region
    dev = regulate_blocks(covs, cut, want_prec=True, engine='device')
    host = regulate_blocks(covs, cut, want_prec=True, engine='host')
    for d, h in zip(dev, host):
        assert 'Wt_dev' in d and d['tri'] == 0                       # (on the device: the parent made these on the host)
        assert d['modes'] == h['modes'] and d['nmod'] == h['nmod'] > 0
        assert d['logdet'] == pytest.approx(h['logdet'], rel=1e-11)
        hp = h['Wt'] @ h['Wt'].T
        assert gu.relmax(d['Wt'] @ d['Wt'].T, hp) < 1e-9
        assert gu.relmax(d['prec'], hp) < 1e-9
        assert gu.relmax(d['S'] @ d['S'].T, h['S'] @ h['S'].T) < 1e-9
        assert d.has_S_add() == h.has_S_add() == (cut > 0)
        if cut > 0:
            assert gu.relmax(d['S_add'] @ d['S_add'].T, h['S_add'] @ h['S_add'].T) < 1e-9
        else:
            assert d['modes'] < B and np.all(d['Wt'][:, d['modes']:] == 0.0)


@pytest.fixture(scope='module')
def rankdef_problem():
    """make_cosmix(N=256, P=16, block=64) with rank-deficient block covariances (and noise drawn from them)"""
    from lsqfit_amd import synth
    d = synth.make_cosmix(N=256, P=16, seed=5, block=64)
    rng = np.random.default_rng(55)
    sig = d['yerr']['sdev']
    ymean = synth.cosmix_f(d['x'], d['p_true'])
    blocks = []
    for r0 in range(0, 256, 64):
        s = sig[r0:r0 + 64]
        c = corr(rankdef(rng, 64)) * np.outer(s, s)
        assert clear_of_floor(c, 1e-3)
        w, v = np.linalg.eigh(c)
        ymean[r0:r0 + 64] += v @ (np.sqrt(np.clip(w, 0.0, None)) * rng.standard_normal(64))
        blocks.append((r0, c))
    return dict(d, ymean=ymean, yerr=dict(sdev=sig, blocks=blocks))


def test_fit_with_device_eigen_whitening(amd, rankdef_problem, monkeypatch):
    d = rankdef_problem
    monkeypatch.setenv('LSQAMD_EIGH', 'device')                     # four blocks: below the crossover
    wd = amd.Whitening(d['ymean'], d['yerr'], *d['prior'], svdcut=1e-3, engine='device')
    wh = amd.Whitening(d['ymean'], d['yerr'], *d['prior'], svdcut=1e-3, engine='host')
    assert all('Wt_dev' in k and k['tri'] == 0 for k in wd.blocks)
    assert wd.nchiv == wh.nchiv and wd.nmod == wh.nmod > 0 and wd.logdet == pytest.approx(wh.logdet, rel=1e-11)
    kw = dict(data=(d['x'], d['ymean'], d['yerr']), model=d['model'], prior=d['prior'], svdcut=1e-3)
    fd = amd.nonlinear_fit(problem=amd.DeviceProblem(d['model'], d['x'], wd), **kw)
    fh = amd.nonlinear_fit(problem=amd.DeviceProblem(d['model'], d['x'], wh), **kw)
    assert gu.relmax(fd.pmean, fh.pmean) < 1e-9 and gu.relmax(fd.cov, fh.cov) < 1e-8
    assert fd.chi2 == pytest.approx(fh.chi2, rel=1e-9) and fd.logGBF == pytest.approx(fh.logGBF, rel=1e-9)
    ref = gu.oracle_fit(d, solver='cholesky', svdcut=1e-3)
    assert gu.relmax(fd.pmean, ref.pmean) < 1e-6 and gu.relmax(fd.cov, ref.cov) < 1e-6


def test_stacked_whitenings_stay_on_the_device(amd, rankdef_problem, monkeypatch):
    monkeypatch.setenv('LSQAMD_EIGH', 'device')
    import torch
    from lsqfit_amd.whiten import stack_whitenings
    d = rankdef_problem
    rng = np.random.default_rng(56)
    sig = d['yerr']['sdev']
    yerrs = []
    for _ in range(4):
        blocks = [(r0, corr(rankdef(rng, 64)) * np.outer(sig[r0:r0 + 64], sig[r0:r0 + 64])) for r0 in range(0, 256, 64)]
        assert all(clear_of_floor(c, 1e-3) for _, c in blocks)
        yerrs.append(dict(sdev=sig, blocks=blocks))
    bd = stack_whitenings(d['ymean'], yerrs, svdcut=1e-3, engine='device')
    bh = stack_whitenings(d['ymean'], yerrs, svdcut=1e-3, engine='host')
    assert isinstance(bd.wt, torch.Tensor) and bd.wt.is_cuda and not np.any(bd.tri)
    assert np.array_equal(bd.modes, bh.modes) and np.allclose(bd.logdet_data, bh.logdet_data, rtol=1e-11, atol=0)
    wd, whh = bd.wt.cpu().numpy().reshape(4, 4, 64, 64), bh.wt.reshape(4, 4, 64, 64)
    for b in range(4):
        for j in range(4):
            assert gu.relmax(wd[b, j] @ wd[b, j].T, whh[b, j] @ whh[b, j].T) < 1e-9


def test_refusals_and_fallbacks(amd, monkeypatch):
    from lsqfit_amd.whiten import regulate_blocks
    monkeypatch.setenv('LSQAMD_EIGH', 'device')
    bad = gap(np.random.default_rng(11), 8)
    bad[0, 1] = bad[1, 0] = 2.0 * np.sqrt(bad[0, 0] * bad[1, 1])     # a correlation of 2: indefinite
    with pytest.raises(ValueError, match='positive definite'):
        regulate_blocks([bad], 0.0, engine='device')
    assert clear_of_floor(bad, 1e-3)
    d, h = (regulate_blocks([bad], 1e-3, engine=e)[0] for e in ('device', 'host'))
    assert 'Wt_dev' in d and d['nmod'] == h['nmod'] and d['logdet'] == pytest.approx(h['logdet'], rel=1e-11)
    assert gu.relmax(d['Wt'] @ d['Wt'].T, h['Wt'] @ h['Wt'].T) < 1e-9
    big = rankdef(np.random.default_rng(257), 257)                   # above the device solver's range: LAPACK, the host's numbers
    d, h = (regulate_blocks([big], 1e-3, engine=e)[0] for e in ('device', 'host'))
    assert 'Wt_dev' not in d and np.array_equal(d['Wt'], h['Wt']) and d['logdet'] == h['logdet']
    c = whitening_inputs(64)[0]
    for knob in ('host', None):                                      # the old routing; one block is below the crossover
        monkeypatch.setenv('LSQAMD_EIGH', knob) if knob else monkeypatch.delenv('LSQAMD_EIGH')
        d, h = (regulate_blocks([c], 1e-3, engine=e)[0] for e in ('device', 'host'))
        assert 'Wt_dev' not in d and np.array_equal(d['Wt'], h['Wt']) and d['nmod'] == h['nmod']
