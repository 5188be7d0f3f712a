"""-m gpu: the K-stage loops of gemm_tn_f64.hip (gemm_tn_f64_interior_kernel, whiten_synth_kernel) at the edges of their
control flow.  The loops run unrolled by two over compile-time LDS buffers with a peeled last stage, and the triangular
stages of the whitening product are split from the full ones, so the cases here are chosen by STAGE COUNT:

 * J^T J (the work-list instantiations): per-entry stage counts 1, 2, odd >= 3, even >= 4, a shorter last K-chunk, entries
   without rows, against numpy with the forward bound of an N-term dot product;
 * the whitening product: blocks of 1 .. 8 tile rows (only triangular stages, the bench shape, unpaired, paired, a middle
   row inside a paired launch, the two-kernel route), both synthesis tile widths, both trig variants, the synthesising
   route bit-equal to the two-kernel one and both within the bound of a B-term dot product of numpy's W_b @ Jraw_b;
 * the batched instantiation with a fit masked out by batch_active.

Bounds: gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1): what ANY order of
summation of an n-term fp64 dot product satisfies, elementwise against |a|^T |b|.  References are formed in long double."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble


def gamma(n):
    return n * U / (1.0 - n * U)


def ld_matmul(a, b):
    """a @ b accumulated in long double (x86: 64-bit mantissa, its own error 2^-11 of the bounds used here)."""
    return np.asarray(a, LD) @ np.asarray(b, LD)


def cosmix_jac(x, p):
    K = p.size // 2
    wx = np.outer(x, p[K:])
    return np.hstack([np.cos(wx), (-p[:K] * x[:, None]) * np.sin(wx)])


def multiexp_jac(x, p):
    K = p.size // 2
    e = np.exp(-np.outer(x, p[K:]))
    return np.hstack([e, (-p[:K] * x[:, None]) * e])


@pytest.fixture(scope='module')
def amd():
    import lsqfit_amd
    from lsqfit_amd import _lib
    _lib.load()
    return lsqfit_amd


# ---- J^T J: stage counts of the split-K work list ---------------------------------------------------------------------------

def stage_counts(N, splits):
    """K stages (16 rows each) of the entries of split 0 .. splits - 1, as launch_gemm_tn cuts N rows into K-chunks."""
    kchunk = -(-N // splits)
    kchunk = max(-(-kchunk // 16) * 16, 16)
    return [max(0, min(s * kchunk + kchunk, N) - s * kchunk) // 16 for s in range(splits)]


PRODUCT_ROWS = (16, 32, 48, 64, 208, 4112)


@pytest.mark.parametrize('P', [128, 256, 384])
def test_product_stage_count_edges(amd, P):
    from lsqfit_amd import synth
    seen = []
    for N in PRODUCT_ROWS:
        if N > 1000 and P > 128:
            continue                      # (the long case once: its long double reference is the slow part)
        d = synth.make_cosmix(N=N, P=P, seed=1000 + N + P, block=0)
        wh = amd.Whitening(d['ymean'], d['yerr'])                      # diagonal data covariance, no prior: A = J^T J
        pr = amd.DeviceProblem(d['model'], d['x'], wh)
        p = d['p_true'] * (1.0 + 1e-3 * np.random.default_rng(N).standard_normal(P))
        chi2 = pr.normal(p)
        splits = (pr.lib.lsqamd_debug_flags(pr.h) >> 8) & 0xffffff
        counts = stage_counts(N, splits)
        seen.append(counts)
        A, g, J, f = pr.get_jtj(), pr.get_grad(), pr.get_J_data(), pr.get_f_data()
        pr.close()
        assert J.shape == (N, P) and f.shape == (N,) and sum(counts) == N // 16
        absJ = np.abs(J)
        errA = np.abs(np.asarray(A, LD) - ld_matmul(J.T, J))
        boundA = gamma(N) * ld_matmul(absJ.T, absJ)
        errg = np.abs(np.asarray(g, LD) - ld_matmul(J.T, f))
        boundg = 1e-12 * ld_matmul(absJ.T, np.abs(f))                 # (gamma_N <= 4.6e-13 for these N)
        chi2_ref = float(ld_matmul(f, f))
        print('P %d N %d splits %d stages %s: max |dA| / bound %.3g, max |dg| / (1e-12 |J|^T |f|) %.3g, chi2 rel %.3g' % (
            P, N, splits, sorted(set(counts)), float(np.max(errA / boundA)), float(np.max(errg / boundg)),
            abs(chi2 - chi2_ref) / chi2_ref))
        assert np.all(errA <= boundA), (N, float(np.max(errA / boundA)))
        assert np.all(errg <= boundg), (N, float(np.max(errg / boundg)))
        assert abs(chi2 - chi2_ref) <= 1e-12 * chi2_ref
    flat = [c for counts in seen for c in counts]
    assert 1 in flat and 2 in flat
    assert any(c >= 3 and c % 2 == 1 for c in flat) and any(c >= 4 and c % 2 == 0 for c in flat)
    # a last K-chunk shorter than the others
    assert any(len(nz) >= 2 and nz[-1] < nz[0] for nz in ([c for c in counts if c > 0] for counts in seen))


# ---- whitening product: triangular stages -----------------------------------------------------------------------------------

# (name, model, block rows, blocks): 1 .. 8 tile rows of 128
TRI_CASES = [('%s%d' % (m, B), m, B, nb) for m in ('cos', 'mexp')
             for B, nb in ((128, 2), (256, 2), (384, 2), (512, 2), (640, 1), (1024, 1))]
TRI_P = 128
BIG_N, BIG_B = 65536, 256      # N * P / 2 = 2^22: from here on the handle keeps a trig range flag (the far-range-free kernel)


def tri_problem(model, B, nb):
    """-> dict(model, x, ymean, yerr, p, jac): nb covariance blocks of B rows covering every row, P = 128."""
    import lsqfit_amd as amd
    from lsqfit_amd import synth
    N, K = B * nb, TRI_P // 2
    if model == 'cos':
        d = synth.make_cosmix(N=N, P=TRI_P, seed=B + nb, block=B)
        p = d['p_true'] * (1.0 + 1e-3 * np.random.default_rng(B).standard_normal(TRI_P))
        return dict(model=d['model'], x=d['x'], ymean=d['ymean'], yerr=d['yerr'], p=p, jac=cosmix_jac)
    rng = np.random.default_rng(B + 7 * nb)
    x = np.linspace(0.05, 3.0, N)
    pt = np.concatenate([rng.uniform(0.5, 1.5, K), 0.05 * np.arange(1, K + 1)])
    y = np.exp(-np.outer(x, pt[K:])) @ pt[:K]
    sd = 0.01 * np.abs(y)
    blocks = [(r0, np.diag(sd[r0:r0 + B] ** 2) + 0.3 * np.outer(sd[r0:r0 + B], sd[r0:r0 + B])) for r0 in range(0, N, B)]
    return dict(model=amd.multiexp(K), x=x, ymean=y, yerr=dict(sdev=sd, blocks=blocks), p=pt * 1.01, jac=multiexp_jac)


def big_problem():
    """The bench shape's structure at P = 128: 256 blocks of 256 rows (one correlation matrix, scaled per block)."""
    import lsqfit_amd as amd
    N, B, K = BIG_N, BIG_B, TRI_P // 2
    rng = np.random.default_rng(99)
    x = np.arange(N) * (2 * np.pi / N)
    pt = np.concatenate([rng.uniform(0.5, 1.5, K), np.arange(1, K + 1) + rng.uniform(-0.05, 0.05, K)])
    y = np.cos(np.outer(x, pt[K:])) @ pt[:K]
    sd = 1e-3 * np.abs(y)
    sd[sd <= 0] = sd[sd > 0].min()
    Um = rng.uniform(0.1, 0.9, (B, 2 * B))
    corr = Um @ Um.T
    dd = 1.0 / np.sqrt(np.diag(corr))
    corr *= np.outer(dd, dd)
    blocks = [(r0, corr * np.outer(sd[r0:r0 + B], sd[r0:r0 + B])) for r0 in range(0, N, B)]
    p = pt * (1.0 + 1e-3 * rng.standard_normal(TRI_P))
    p_far = p.copy()
    p_far[-1] = 4.0e13         # |w x| up to 2.5e14: past the 1e13 limit of the fast trig reduction -> the range flag is set
    return dict(model=amd.cosmix(K), x=x, ymean=y + sd * rng.standard_normal(N), yerr=dict(sdev=sd, blocks=blocks), p=p,
                p_far=p_far, jac=cosmix_jac)


def route_main(path, save_w):
    """(child process, one route: LSQAMD_FUSED_JACOBIAN and LSQAMD_SYNTH_NARROW are set by the parent) the whitened Jacobian
    and J^T J of every case; the whitening matrices themselves from the child that is asked for them, their digests from all."""
    import lsqfit_amd as amd
    out = {}

    def weights(name, wh, which):
        assert all(int(k['tri']) == 1 and int(k['modes']) == int(k['size']) for k in wh.blocks), name
        h = hashlib.sha256()
        for i, k in enumerate(wh.blocks):
            W = np.ascontiguousarray(k['Wt'].T)
            h.update(W.tobytes())
            if save_w and i in which:
                out['%s_W%d' % (name, i)] = W
        out[name + '_Wsha'] = h.hexdigest()

    for name, model, B, nb in TRI_CASES:
        d = tri_problem(model, B, nb)
        wh = amd.Whitening(d['ymean'], d['yerr'])
        pr = amd.DeviceProblem(d['model'], d['x'], wh)
        out[name + '_chi2'] = pr.normal(d['p'])
        out[name + '_J'], out[name + '_A'] = pr.get_J_data(), pr.get_jtj()
        out[name + '_synth'] = bool(pr.lib.lsqamd_debug_flags(pr.h) & 2)
        pr.close()
        weights(name, wh, range(nb))
    d = big_problem()
    wh = amd.Whitening(d['ymean'], d['yerr'])
    pr = amd.DeviceProblem(d['model'], d['x'], wh)
    ends = np.r_[0:BIG_B, BIG_N - BIG_B:BIG_N]
    for name, p in (('big', d['p']), ('bigfar', d['p_far'])):
        out[name + '_chi2'] = pr.normal(p)
        J = pr.get_J_data()
        out[name + '_Jsha'] = hashlib.sha256(np.ascontiguousarray(J).tobytes()).hexdigest()
        out[name + '_J'], out[name + '_A'] = J[ends].copy(), pr.get_jtj()
        out[name + '_synth'] = bool(pr.lib.lsqamd_debug_flags(pr.h) & 2)
    pr.close()
    weights('big', wh, (0, BIG_N // BIG_B - 1))
    np.savez(path, **out)


_ROUTES = {}


def route(tmp_factory, fused, narrow):
    key = (fused, narrow)
    if key not in _ROUTES:
        path = str(tmp_factory.mktemp('stage_loops') / ('route_%d_%d.npz' % key))
        env = dict(os.environ, LSQAMD_FUSED_JACOBIAN=str(fused), LSQAMD_SYNTH_NARROW='1000000' if narrow else '0')
        code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_stage_loops import route_main; route_main(%r, %r)' % (
            ROOT, path, key == (1, 0))
        r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _ROUTES[key] = dict(np.load(path))
    return _ROUTES[key]


_REFS = {}


def references(tmp_factory):
    """name -> (W_b @ Jraw_b in long double, gamma_B |W_b| |Jraw_b|) of the rows kept in '<name>_J': once, from the whitening
    matrices of the (fused, wide) child; every other child must have made the same matrices."""
    if not _REFS:
        r = route(tmp_factory, 1, 0)
        for name, model, B, nb in TRI_CASES:
            d = tri_problem(model, B, nb)
            ref, bound = [], []
            for b in range(nb):
                W, Jraw = r['%s_W%d' % (name, b)], d['jac'](d['x'][b * B:(b + 1) * B], d['p'])
                ref.append(ld_matmul(W, Jraw))
                bound.append(gamma(B) * ld_matmul(np.abs(W), np.abs(Jraw)))
            _REFS[name] = (np.vstack(ref), np.vstack(bound))
        d = big_problem()
        for name, p in (('big', d['p']), ('bigfar', d['p_far'])):
            ref, bound = [], []
            for b in (0, BIG_N // BIG_B - 1):
                W, Jraw = r['big_W%d' % b], d['jac'](d['x'][b * BIG_B:(b + 1) * BIG_B], p)
                ref.append(ld_matmul(W, Jraw))
                bound.append(gamma(BIG_B) * ld_matmul(np.abs(W), np.abs(Jraw)))
            _REFS[name] = (np.vstack(ref), np.vstack(bound))
    return _REFS


ALL_TRI = [c[0] for c in TRI_CASES] + ['big', 'bigfar']


@pytest.mark.parametrize('narrow', [0, 1])
def test_triangular_stages_routes_bit_equal(tmp_path_factory, narrow):
    a, b = route(tmp_path_factory, 1, narrow), route(tmp_path_factory, 0, narrow)
    for name in ALL_TRI:
        B = dict((c[0], c[2]) for c in TRI_CASES).get(name, BIG_B)
        # (blocks of eight tile rows and more take the two-kernel route either way: gemm_tn_f64.hip whiten_synth_eligible)
        assert bool(a[name + '_synth']) == (B < 1024) and not bool(b[name + '_synth']), name
        assert np.array_equal(a[name + '_J'], b[name + '_J']), name
        assert np.array_equal(a[name + '_A'], b[name + '_A']), name
        if name + '_Jsha' in a:
            assert str(a[name + '_Jsha']) == str(b[name + '_Jsha']), name
    for name in [c[0] for c in TRI_CASES] + ['big']:
        assert str(a[name + '_Wsha']) == str(b[name + '_Wsha']) == str(route(tmp_path_factory, 1, 0)[name + '_Wsha']), name


@pytest.mark.parametrize('fused,narrow', [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_triangular_stages_against_numpy(tmp_path_factory, fused, narrow):
    refs, r = references(tmp_path_factory), route(tmp_path_factory, fused, narrow)
    worst = {}
    for name in ALL_TRI:
        ref, bound = refs[name]
        J = r[name + '_J']
        assert J.shape == ref.shape and np.all(np.isfinite(J)), name
        err = np.abs(np.asarray(J, LD) - ref)
        # (the cosine model's first row has x = 0: its frequency derivatives and their bound are exactly zero, and so is J)
        nz = bound > 0
        worst[name] = (float(np.max(err[nz] / bound[nz])), bool(np.all(err <= bound)))
    print('fused %d narrow %d: max |dJ| / (gamma_B |W| |Jraw|): %s' % (fused, narrow,
                                                                       ' '.join('%s %.3g' % (k, v[0]) for k, v in worst.items())))
    assert all(v[1] for v in worst.values()), worst


# ---- the batched instantiation ------------------------------------------------------------------------------------------------

def test_batched_product_with_a_fit_masked_out(amd):
    """Three lockstep fits of (256, 128); the third starts at its own solution and is done rounds before the others, so the
    batched J^T J launches that follow skip it (batch_active)."""
    from lsqfit_amd import synth
    from tests import gpu_util as gu
    d = synth.make_cosmix(N=256, P=128, seed=61, block=0)
    pm, ps = d['prior']
    pmb, psb = np.tile(pm, (3, 1)), np.tile(ps, (3, 1))
    psb[1, :64] = 0.2
    kw = dict(data=(d['x'], d['ymean'], d['yerr']), model=d['model'])
    p0 = np.tile(d['p0'], (3, 1))
    p0[1] += 0.01
    p0[2] = amd.nonlinear_fit(prior=(pmb[2], psb[2]), p0=p0[2], **kw).pmean
    singles = [amd.nonlinear_fit(prior=(pmb[b], psb[b]), p0=p0[b], **kw) for b in range(3)]
    bf = amd.BatchedFits(d['model'], d['x'], d['ymean'], d['yerr'], pmb, psb)
    out = bf.run(p0=p0)
    bf.close()
    print('nit batched %s single %s' % (out['nit'], [s.nit for s in singles]))
    assert np.all(out['status'] == 0)
    assert out['nit'][2] < min(out['nit'][0], out['nit'][1])          # a fit finished at least a round early
    for b in range(3):
        assert out['nit'][b] == singles[b].nit
        assert gu.relmax(out['pmean'][b], singles[b].pmean) < 1e-10
        assert out['chi2'][b] == pytest.approx(singles[b].chi2, rel=1e-10)
