"""The parabola step that ends a scalar ``empbayes_fit`` search (sweep.refine_scalar), with a stand-in fitter (no device)."""
import numpy as np

from lsqfit_amd.sweep import EvidenceSurface, empbayes_fit, refine_scalar, simplex_search


class FakeFit:
    """logGBF(z) of the shape the data-error search of the reference's eg7 has: -n log z - a / z^2 (+ constant), peak at
    z* = sqrt(2 a / n)"""
    N, A = 4.0, 4.0 * 0.015676298783 ** 2 / 2.0

    def __init__(self, z, **kw):
        self.logGBF = -self.N * np.log(z) - self.A / z ** 2
        self.pmean = np.array([z])


def fitargs(z):
    return dict(z=z)


def test_refinement_puts_z_well_inside_tol():
    zstar = np.sqrt(2.0 * FakeFit.A / FakeFit.N)
    tol = 1e-6
    surface = EvidenceSurface(fitargs, scalar=True, fitter=lambda **kw: FakeFit(**kw))
    simplex_search(surface, np.array([0.001]), tol=tol)
    z_search, f_search = float(surface.zbest[0]), surface.fbest
    assert abs(z_search - zstar) <= tol                       # what the search's stopping rule promises
    refine_scalar(surface, tol)
    z_ref = float(surface.zbest[0])
    # the parabola's own error: the cubic term (d^2 + 3 e^2) |f'''| / (6 f'') with d = 8 tol, the stencil's centre e <= tol
    # beside the optimum, |f'''| / f'' = 5 / z* for this shape; 1e-12 for the rounding of the three values
    bound = ((8 * tol) ** 2 + 3 * tol ** 2) * 5.0 / zstar / 6.0 + 1e-12
    print('search %.3e, refined %.3e, bound %.3e' % (abs(z_search - zstar), abs(z_ref - zstar), bound))
    assert abs(z_ref - zstar) <= bound < 1e-2 * tol
    assert surface.fbest <= f_search                          # never a higher value
    fit, z = empbayes_fit(0.001, fitargs, tol=tol, fitter=lambda **kw: FakeFit(**kw))
    assert z == z_ref and fit.logGBF == -surface.fbest


def test_refinement_leaves_a_surface_that_is_no_bowl_alone():
    class Line:
        def __init__(self, z, **kw):
            self.logGBF, self.pmean = z, np.array([z])
    surface = EvidenceSurface(fitargs, scalar=True, fitter=lambda **kw: Line(**kw))
    surface(np.array([[1.0]]))
    refine_scalar(surface, 1e-3)
    assert surface.nfits == 3 and float(surface.zbest[0]) == 1.0 + 8e-3      # the two side points only; the lower one is kept
