"""A plain NumPy restatement of the reference's Kurganov-Tadmor scheme (kurganov_tadmor,
fluid.py:103-464; at_interface, slope_ratio, kurganov_tadmor_flux, finalize_rk_step and the flux
limiters, fluid.py:466-673), shared by tests/test_fluid_kt_host.py and tests/test_gpu_fluid_kt.py.

The reference loops over the variable, then the direction, then the interfaces [i-½, j, k] in
ascending (i, j, k), and scatters Δ to the two cells beside every interface.  Here the loops over
the variable and the direction are the reference's; the interfaces of one such pass are taken as
one array, which keeps the order of every cell's own sums: `new += Δ` is the interface below the
cell (index_c, reached first), `new -= roll(Δ, -1)` the one above it (index_m of the next
interface).  Periodic neighbours by np.roll; every expression with the reference's parentheses;
the branches by np.where over the values of all branches."""
import numpy as np

machine_ϵ = float(np.finfo(np.float64).eps)
slope_ratio_ϵ = 1e+2*machine_ϵ
β_sweby = 1.5

# flux_limiter_select -> the limiter, with the reference's aliases (fluid.py:208-227)
ALIASES = {'mc': 'monotonizedcentral', 'muscl': 'vanleer', 'harmonic': 'vanleer'}


def slope_ratio(numerator, denominator):
    numerator, denominator = np.asarray(numerator, float), np.asarray(denominator, float)
    with np.errstate(all='ignore'):
        out = numerator/denominator
    small = np.abs(denominator) < slope_ratio_ϵ
    out = np.where(small & (numerator < -slope_ratio_ϵ), -1/slope_ratio_ϵ, out)
    out = np.where(small & (numerator > slope_ratio_ϵ), 1/slope_ratio_ϵ, out)
    return np.where(np.abs(numerator) < slope_ratio_ϵ, 0.0, out)


def _branches(r, *pairs):
    """the value of the first (condition, value) pair whose condition holds, else 0"""
    out = np.zeros_like(r)
    for condition, value in reversed(pairs):
        out = np.where(condition, value, out)
    return out


def limiter(name):
    name = ALIASES.get(name, name)

    def ϕ(r):
        r = np.asarray(r, float)
        with np.errstate(all='ignore'):
            if name == 'minmod':
                return _branches(r, (r > 1, 1.0), (r > 0, r))
            if name == 'monotonizedcentral':
                return _branches(r, (r > 3, 2.0), (r > 1./3., 0.5*(r + 1)), (r > 0, 2*r))
            if name == 'ospre':
                r2 = r*r
                return _branches(r, (r > 0, 1.5*(r2 + r)/((r2 + r) + 1)))
            if name == 'superbee':
                return _branches(r, (r > 2, 2.0), (r > 1, r), (r > 0.5, 1.0), (r > 0, 2*r))
            if name == 'sweby':
                return _branches(r, (r > β_sweby, β_sweby), (r > 1, r), (r > 1/β_sweby, 1.0),
                                 (r > 0, β_sweby*r))
            if name == 'umist':
                return _branches(r, (r > 5, 2.0), (r > 1, 0.75 + 0.25*r),
                                 (r > 0.2, 0.25 + 0.75*r), (r > 0, 2*r))
            if name == 'vanalbada':
                r2 = r*r
                return _branches(r, (r > 0, (r2 + r)/(r2 + 1)))
            if name == 'vanleer':
                return _branches(r, (r > 0, 2*r/(1 + r)))
            if name == 'koren':
                return _branches(r, (r > 2.5, 2.0), (r > 0.25, 1./3.*(1 + 2*r)), (r > 0, 2*r))
        raise ValueError(f'Flux limiter "{name}" not implemented')
    ϕ(0.0)
    return ϕ


def at_interface(q, axis, ϕ):
    """the left and right value at the interface below every cell along axis"""
    m2, m, c, p = np.roll(q, 2, axis), np.roll(q, 1, axis), q, np.roll(q, -1, axis)
    r_m = slope_ratio(m - m2, c - m)
    r_c = slope_ratio(c - m, p - c)
    return m + 0.5*ϕ(r_m)*(c - m), c - (0.5*ϕ(r_c))*(p - c)


def pairmax(a, b):
    return a*(b <= a) + b*(a < b)


def kt_flux(q, f, v):
    speed = pairmax(v[0], v[1])
    return 0.5*((f[1] + f[0]) - speed*(q[1] - q[0]))


def kt_step_np(src, dst, rk_step, rk_order, ϕ, k):
    """One Runge-Kutta step.  src: [ϱ, Jx, Jy, Jz] as the stencil reads them, dst: the grids the
    step adds to (used in step 1 only).  k: a dict of c2w, inv_c2, a_pow, soundspeed, f_J, f_P,
    Δt_over_Δx.  Returns (the four grids written, 𝒫 as realised)."""
    ϱ, J = src[0], src[1:]
    𝒫 = ϱ*k['c2w']
    new = [np.zeros_like(ϱ) for _ in range(4)] if rk_step == 0 else [np.array(d) for d in dst]
    to_delta = (1 + rk_step)/rk_order*k['Δt']/k['Δx']
    use_𝒫 = k['c2w'] != 0
    with np.errstate(all='ignore'):
        for m in range(3):
            ϱ_i, 𝒫_i, Jm_i = (at_interface(x, m, ϕ) for x in (ϱ, 𝒫, J[m]))
            v = [np.abs(k['a_pow']*Jm_i[lr]/(ϱ_i[lr] + k['inv_c2']*𝒫_i[lr])) + k['soundspeed']
                 for lr in range(2)]
            f = [k['f_J']*Jm_i[lr] for lr in range(2)]
            Δ = kt_flux(ϱ_i, f, v)*to_delta
            new[0] += Δ
            new[0] -= np.roll(Δ, -1, m)
        for m in range(3):
            for n in range(3):
                ϱ_i, 𝒫_i, Jm_i, Jn_i = (at_interface(x, n, ϕ) for x in (ϱ, 𝒫, J[m], J[n]))
                v = [np.abs(k['a_pow']*Jn_i[lr]/(ϱ_i[lr] + k['inv_c2']*𝒫_i[lr]))
                     + k['soundspeed'] for lr in range(2)]
                f = [k['f_J']*(Jm_i[lr]*Jn_i[lr]/(ϱ_i[lr] + k['inv_c2']*𝒫_i[lr]))
                     for lr in range(2)]
                if use_𝒫 and m == n:
                    f = [f[lr] + k['f_P']*𝒫_i[lr] for lr in range(2)]
                Δ = kt_flux(Jm_i, f, v)*to_delta
                new[1 + m] += Δ
                new[1 + m] -= np.roll(Δ, -1, n)
    if rk_step == 0:
        new = [x + s for x, s in zip(new, src)]
    return new, 𝒫


def factors(light_speed, w, a, Δx, Δt, dt_J, dt_P):
    """the reference's ℝ[...] expressions of one step at scale factor a (w_eff = w)"""
    return {'c2w': light_speed**2*w, 'inv_c2': light_speed**(-2), 'a_pow': a**(3*w - 2),
            'soundspeed': light_speed*np.sqrt(w)/a, 'f_J': dt_J/Δt,
            'f_P': dt_P/Δt if w != 0 else 0.0, 'Δt': Δt, 'Δx': Δx}


def kt_np(ϱ, J, *, light_speed, w, Δx, Δt, dt_J, dt_P, a_steps, rk_order, limiter_name):
    """One kurganov_tadmor() call.  a_steps: the scale factor of every Runge-Kutta step.
    Returns (ϱ, J stacked, 𝒫 as the call leaves it)."""
    ϕ = limiter(limiter_name)
    grids = [np.array(ϱ, dtype=np.float64)] + [np.array(j, dtype=np.float64) for j in J]
    assert len(a_steps) == rk_order
    k = factors(light_speed, w, float(a_steps[0]), Δx, Δt, dt_J, dt_P)
    starred, 𝒫 = kt_step_np(grids, None, 0, rk_order, ϕ, k)
    if rk_order == 1:
        grids = starred
    else:
        k = factors(light_speed, w, float(a_steps[1]), Δx, Δt, dt_J, dt_P)
        grids, 𝒫 = kt_step_np(starred, grids, 1, rk_order, ϕ, k)
    return grids[0], np.stack(grids[1:]), 𝒫


def kt_np_of_golden(g, ϱ, J, row, a_steps):
    """kt_np with the settings of a golden; row: (ᔑdt['1'], ['a**(3*w_eff-2)'], ['a**(-3*w_eff)'])"""
    return kt_np(ϱ, J, light_speed=float(g['light_speed']), w=float(g['w']),
                 Δx=float(g['boxsize'])/int(g['gridsize']), Δt=float(row[0]), dt_J=float(row[1]),
                 dt_P=float(row[2]), a_steps=a_steps, rk_order=int(g['rk_order']),
                 limiter_name=str(g['limiter']))
