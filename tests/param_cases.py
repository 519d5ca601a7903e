"""The contact-model parameter sets of the tests that leave the synthetic default (kuhn 1, lm 9.6, slope -1.5, d 3): what a fit
(rippe_fit.estimate_param_rippe) and the nuisance steps behind every MCMC step hand to the kernels, and the two signs of d - 2 the default
never shows.  `with_params` puts a set behind a problem WITHOUT touching its contacts -- the nuisance step's situation -- and keeps the
problem's own fact, v_inter and (where it set one) d_max, so its windows, tiles and branch reach stay what the case was built for.

The preconditions below are asserted on the CPU (tests/test_ref_kernels_cpu.py, tests/test_sparse_reformulation.py) and again in front of
every GPU launch (tests/test_model_params_gpu.py), so that a set cannot quietly empty a comparison: a case that breaks one gets another
fact, never a skip.

Nothing here needs a device."""
import numpy as np

from graal_amd import synth

#            kuhn  lm    slope  d
SETS = {
    "fitted_a": dict(kuhn=0.82, lm=11.3, slope=-1.13, d=3.0),    # the division branch of rippe, a shallow slope
    "fitted_b": dict(kuhn=2.5, lm=6.0, slope=-2.2, d=3.0),       # the division branch, a steep slope, kuhn > 1
    "d_below_2": dict(kuhn=1.0, lm=9.6, slope=-1.5, d=0.5),      # d - 2 < 0: the exponential grows with distance
    "d_is_2": dict(kuhn=0.7, lm=14.0, slope=-0.75, d=2.0),       # the exponent exactly 0, the division branch
}
NAMES = tuple(SETS)
FITTED = ("fitted_a", "fitted_b")
FIXED_POINT_LIMIT = 2.0 ** 31      # a pair that expects this many contacts does not fit the maps' fixed point (window_cases.m3)

I_KUHN, I_LM, I_C1, I_SLOPE, I_D, I_DMAX, I_FACT, I_VINTER = range(8)


def _shape_of(par):
    return dict(kuhn=float(par[I_KUHN]), lm=float(par[I_LM]), slope=float(par[I_SLOPE]), d=float(par[I_D]))


def bisected(par):
    """True where the parameter vector's d_max is the one synth.make_param_simu finds by bisection (the case left it to the model)."""
    par = np.asarray(par, np.float32)
    again = synth.make_param_simu(fact=float(par[I_FACT]), v_inter=float(par[I_VINTER]), **_shape_of(par))
    return again[I_DMAX] == par[I_DMAX]


def param(name, own, fact=None, v_inter=None, d_max=None):
    """The set `name` behind a case whose parameter vector is `own`: fact and v_inter are the case's unless given; d_max is the given one,
    else the case's own where the case set one, else the bisection's under the new set."""
    own = np.asarray(own, np.float32)
    fact = float(own[I_FACT]) if fact is None else fact
    v_inter = float(own[I_VINTER]) if v_inter is None else v_inter
    if d_max is None and not bisected(own):
        d_max = float(own[I_DMAX])
    par = synth.make_param_simu(fact=fact, v_inter=v_inter, d_max=d_max, **SETS[name])
    assert_not_default(par)
    return par


def with_params(P, name, fact=None, v_inter=None, d_max=None):
    """dict(P, param_simu=...): the problem under the set `name`, contacts, layout and everything else untouched."""
    return dict(P, param_simu=param(name, P["param_simu"], fact, v_inter, d_max))


# ---- preconditions ------------------------------------------------------------------------------------------------------------------
def assert_not_default(par):
    """The set is not the one every other test runs under, and is one a kernel can price at all."""
    par = np.asarray(par, np.float32)
    default = synth.make_param_simu()
    assert par.shape == (8,) and par.dtype == np.float32 and np.all(np.isfinite(par))
    assert not np.array_equal(par[[I_KUHN, I_LM, I_SLOPE, I_D]], default[[I_KUHN, I_LM, I_SLOPE, I_D]]), "the default set"
    assert par[I_KUHN] > 0 and par[I_LM] > 0 and par[I_DMAX] > 0 and par[I_VINTER] > 0


def assert_reference_usable(values, what=""):
    """A reference result is finite and not all zero: the comparison that follows compares something."""
    v = np.asarray(values, np.float64)
    assert v.size and np.all(np.isfinite(v)), ("a reference value is not finite", what)
    assert np.any(v != 0), ("the reference is all zero", what)


def assert_fits_fixed_point(expected, what=""):
    """No pair's expected number of contacts reaches the fixed point's 2^31."""
    v = np.asarray(expected, np.float64)
    assert_reference_usable(v, what)
    assert v.max() < FIXED_POINT_LIMIT, ("a pair expects 2^31 contacts or more: give the case another fact", what, v.max())


def assert_no_status(status, nonfinite, what=""):
    """No entry of a scorer's status vector is its NONFINITE."""
    assert not np.any(np.asarray(status) == nonfinite), ("a NONFINITE status under this set", what)


def worst_ratio(err, tol):
    """max |engine - reference| / tolerance, for the margins DESIGN.md section 7 records."""
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    return float(np.max(err / np.maximum(tol, np.finfo(np.float64).tiny))) if err.size else 0.0
