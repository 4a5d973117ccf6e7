"""A plain NumPy and `decimal` restatement of the six quantities of the reference's measure()
(analysis.py:3860-4230), the formulas only, and what the tests of the GPU path need beside it: exact
sums, the error bound of the double-double reduction, and inputs that a double-precision sum gets
wrong.

Every function takes host arrays of the whole box.  exact=True evaluates a quantity the reference
sums in double (np.sum, a running `+=`) from the exact sum instead and finishes it in decimal: the
value the GPU path is held to."""
import decimal
import fractions
import math

import numpy as np

PREC = 2*17   # the reference's decimal.localcontext(prec=2*17), analysis.py:4031
SQUARES_SEED = 4   # unrepresentable_squares(2**16, 4): np.sum of the squares is off by 1.4 ulp/2


# -- exact sums and the bound of the double-double reduction -------------------------------------
def exact_sum(values, square=False):
    """Σx (or Σx², the squares exact) as a Fraction: the integer mantissas of the values that
    share an exponent are added as Python integers, then the groups"""
    values = np.asarray(values, dtype=np.float64).ravel()
    if values.size == 0:
        return fractions.Fraction(0)
    mantissa, exponent = np.frexp(values)
    mantissa = np.ldexp(mantissa, 53).astype(np.int64).astype(object)
    exponent = exponent.astype(np.int64) - 53
    if square:
        mantissa, exponent = mantissa*mantissa, 2*exponent
    lowest = int(exponent.min())
    total = 0
    for e in np.unique(exponent).tolist():
        total += int(np.sum(mantissa[exponent == e])) << (e - lowest)
    return fractions.Fraction(total)*fractions.Fraction(2)**lowest


def to_decimal(fraction, prec=60):
    with decimal.localcontext() as ctx:
        ctx.prec = prec
        return decimal.Decimal(fraction.numerator)/decimal.Decimal(fraction.denominator)


def ulp(x):
    return math.ulp(x) if math.isfinite(x) else math.inf


def sum_bound(n, abs_sum, exact):
    """|Σ_gpu − Σ_exact| <= n 2⁻¹⁰⁰ Σ|x| + ulp(Σ_exact)/2: n double-double additions at 3u² each
    (u = 2⁻⁵³) with slack, and the rounding of the result to double"""
    return n*fractions.Fraction(1, 2**100)*abs_sum + fractions.Fraction(ulp(float(exact)))/2


def partial_of(values):
    """the six numbers cg_measure_sums leaves for `values`, with exact double-double sums"""
    values = np.asarray(values, dtype=np.float64).ravel()
    out = []
    for square in (False, True):
        total = exact_sum(values, square)
        hi = float(total)
        out += [hi, float(total - fractions.Fraction(hi))]
    out += [float(values.min()) if values.size else math.inf,
            float(np.abs(values).max()) if values.size else 0.0]
    return out


def cancelling_values(n, seed, magnitude=1e16):
    """n values (n even) of about `magnitude` in shuffled ± pairs plus residuals of order 1: the
    exact sum is of order sqrt(n), a double-precision sum returns round-off of order `magnitude`
    ulps"""
    rng = np.random.default_rng(seed)
    big = magnitude*(1 + rng.random(n//2))
    values = np.concatenate([big, -big]) + rng.standard_normal(n)
    rng.shuffle(values)
    return values


def unrepresentable_squares(n, seed):
    """n values with full 53-bit mantissas over a few decades: no square fits a double"""
    rng = np.random.default_rng(seed)
    values = (1 + rng.random(n))*10.0**rng.integers(-3, 6, n)*rng.choice([-1.0, 1.0], n)
    assert all(fractions.Fraction(x)**2 != fractions.Fraction(x*x) for x in values[:64].tolist())
    return values


# -- the quantities ------------------------------------------------------------------------------
def _decimal_sums(values, count, scale=None):
    """(Σ, σ) as the reference accumulates them in decimal (analysis.py:4036-4056, 4067-4090)"""
    with decimal.localcontext() as ctx:
        ctx.prec = PREC
        Σ = Σ2 = decimal.Decimal(0)
        for x in np.asarray(values, dtype=np.float64).ravel().tolist():
            x = decimal.Decimal(x)
            Σ += x
            Σ2 += x**2
        if scale is not None:
            Σ *= decimal.Decimal(scale)
            Σ2 *= decimal.Decimal(scale)**2
        σ2 = Σ2/count - (Σ/count)**2
        σ = decimal.Decimal(0) if σ2 < 0 else σ2.sqrt()
        return float(Σ), float(σ)


def variance_from_partials(partials, count):
    """the variance (a Decimal, negative ones left as they are) as the host finishes it from the
    (hi, lo) pairs of the domains: decimal with 34 digits, the pairs added in domain order"""
    with decimal.localcontext() as ctx:
        ctx.prec = PREC
        Σ = Σ2 = decimal.Decimal(0)
        for hi, lo, hi2, lo2 in (partial[:4] for partial in partials):
            Σ += decimal.Decimal(hi)
            Σ += decimal.Decimal(lo)
            Σ2 += decimal.Decimal(hi2)
            Σ2 += decimal.Decimal(lo2)
        return Σ2/count - (Σ/count)**2


def momentum_particles(mom):
    """(Σmom, σmom) of mom[N, 3]"""
    both = [_decimal_sums(mom[:, dim], mom.shape[0]) for dim in range(3)]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both])


def momentum_fluid(J, boxsize):
    """(Σmom, σmom) of the grids J[3] with the factors Vcell and Vcell²"""
    N_elements = J[0].size
    Vcell = boxsize**3/N_elements
    both = [_decimal_sums(J[dim], N_elements, Vcell) for dim in range(3)]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both])


def rho(ϱ, exact=False):
    """(ϱ_bar, σϱ, ϱ_min), analysis.py:4101-4123"""
    N_elements = ϱ.size
    if not exact:
        Σϱ, Σϱ2 = np.sum(ϱ), np.sum(ϱ**2)
        ϱ_bar = Σϱ/N_elements
        σ2ϱ = Σϱ2/N_elements - ϱ_bar**2
        return ϱ_bar, math.sqrt(max(σ2ϱ, 0)), np.min(ϱ)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ϱ_bar = to_decimal(exact_sum(ϱ))/N_elements
        σ2ϱ = to_decimal(exact_sum(ϱ, square=True))/N_elements - ϱ_bar**2
        return float(ϱ_bar), float(max(σ2ϱ, decimal.Decimal(0)).sqrt()), float(np.min(ϱ))


def mass_particles(a, w_eff, N, mass):
    return a**(-3*w_eff)*N*mass


def mass_fluid(ϱ, a, w_eff, boxsize, exact=False):
    Vcell = boxsize**3/ϱ.size
    return a**(-3*w_eff)*Vcell*(float(exact_sum(ϱ)) if exact else np.sum(ϱ))


def v_particles(mom, a, w_eff, mass):
    """(v_max, v_rms), analysis.py:3902-3910, 3966-3972: a running maximum and a running sum"""
    mom2_max = max(0.0, max((x**2 + y**2 + z**2) for x, y, z in mom.tolist()))
    mom2 = 0.0
    for x in mom.ravel().tolist():
        mom2 += x**2
    factor = a**(2 - 3*w_eff)*mass
    return math.sqrt(mom2_max)/factor, math.sqrt(mom2/mom.shape[0])/factor


def v_fluid(ϱ, 𝒫, J, a, w, w_eff, light_speed, exact=False):
    """(v_max, v_rms) of a fluid with non-linear J, analysis.py:3940-3963, 4000-4023"""
    terms = (J[0]**2 + J[1]**2 + J[2]**2)/(ϱ + light_speed**(-2)*𝒫)**2
    v_max = a**(3*w_eff - 2)*math.sqrt(max(0.0, terms.max())) + light_speed*math.sqrt(w)/a
    if exact:
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            rms = float((to_decimal(exact_sum(terms))/terms.size).sqrt())
    else:
        Σ = 0.0
        for term in terms.ravel().tolist():
            Σ += term
        rms = math.sqrt(Σ/terms.size)
    return v_max, a**(3*w_eff - 2)*rms + light_speed*math.sqrt(w)/a


def discontinuity(grid, h, lo=None, hi=None):
    """(Δdiff_max[3], diff_max[3]) of one grid, analysis.py:4171-4213 with the order-1 branch of
    diff_domaingrid (mesh.py:4961-4965).  lo / hi: the layer below grid[0] and above grid[-1]
    (None: the grid wraps around)."""
    inv_h = 1/h
    below = np.concatenate([grid[-1:] if lo is None else lo[None], grid[:-1]])
    above = np.concatenate([grid[1:], grid[:1] if hi is None else hi[None]])
    Δdiff_max, diff_max = np.zeros(3), np.zeros(3)
    for dim in range(3):
        up = above if dim == 0 else np.roll(grid, -1, axis=dim)
        dn = below if dim == 0 else np.roll(grid, +1, axis=dim)
        fwd = inv_h*(up - grid)
        bwd = inv_h*(grid - dn)
        Δdiff_max[dim] = max(0.0, np.abs(fwd - bwd).max())
        diff_max[dim] = max(0.0, np.abs(fwd).max(), np.abs(bwd).max())
    return Δdiff_max, diff_max


def normalized(Δdiff_max, diff_max):
    return np.array([Δdiff_max[dim]/diff_max[dim] if Δdiff_max[dim] > 0 else 0
                     for dim in range(3)])


FLUIDSCALAR_NAMES = ['<fluidscalar 0[0]>', '<fluidscalar 1[0]>', '<fluidscalar 1[1]>',
                     '<fluidscalar 1[2]>', '<fluidscalar 0[0]>']   # ϱ, Jx, Jy, Jz, 𝒫


def discontinuity_fluid(ϱ, J, 𝒫, boxsize):
    """(names, Δdiff_max_list, Δdiff_max_normalized_list) of a boltzmann_order = 1 fluid"""
    h = boxsize/ϱ.shape[0]
    both = [discontinuity(grid, h) for grid in (ϱ, J[0], J[1], J[2], 𝒫)]
    return list(FLUIDSCALAR_NAMES), [b[0] for b in both], [normalized(*b) for b in both]
