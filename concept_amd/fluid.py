"""concept_amd.fluid — the MacCormack scheme (fluid.py:724-1067, 1079-1363 of the reference) and
the Kurganov-Tadmor scheme (fluid.py:103-673) for fluid components on the GPU (csrc/cg_fluid.hip).

In scope: a fluid with non-linear ϱ and J (boltzmann_order = 1, closure 'truncate') and a
constant equation of state P = wρ (select_eos_w; the reference's w_type 'constant'): the two
MacCormack steps with their vacuum check and correction, the eight-fold cycle of step directions,
v_max with the sound speed and the Courant limit, and for w ≠ 0 the realisation 𝒫 = ϱ c²w and the
pressure term of the Euler equation (realize_𝒫, internal_sources, apply_internal_sources).  A
w = 0 component takes the kernels and launches of the flux terms alone.  Out of scope (the
functions raise and name the missing piece): boltzmann_order > 1 with its non-linear ς and 𝒫,
linear variables realised by CLASS other than the ς of closure 'class' below, a w that is not a
constant number, decaying species (mom_decay_factor).  The Hubble term of the continuity
equation needs approximations['P=wρ'] off, which the reference rules out for this scope
(species.py:1678-1685).
Kurganov-Tadmor, in the same scope: Runge-Kutta orders 1 and 2 and the nine flux limiters, one
launch per Runge-Kutta step with the pressure term in the flux (kurganov_tadmor); no vacuum
correction exists in that scheme.

Closure 'class' (a fluid whose hierarchy is closed by realising ς at every step from its own
non-linear ϱ and the caller's table of transfer-function ratios) is opted into: shear_sources is
the shear term of the Euler equation, ΔJⁱ = -ᔑa**(-3*w_eff)dt ∂ʲςⁱⱼ, with the divergence formed in
Fourier space (csrc/cg_lpt.hip), closure_sources / closure_hooks the hooks of the time loop that
know it, and the functions of the MacCormack path take closure_class=True.  Without the keyword
the closure is refused as before; with it boltzmann_order ≠ 1, the P=wρ approximation off, a
structure other than 'nonlinear', Kurganov-Tadmor and several domains are refused by name.

Use is explicit — nothing calls this module on its own:

    stepper.Timeloop(comps, fluid_drift=fluid.drift, fluid_limiter=fluid.courant_limit,
                     fluid_sources=fluid.apply_internal_sources)   # the last for w ≠ 0

drift() and apply_internal_sources() are the MacCormack scheme and refuse any other;
drift_selected() and sources_selected() take their place in the call above to send every
component to the scheme fluid_scheme_select names for it.

The starred grids of a component, its fac_time grid and the device flag are allocated on its
first maccormack(), the Δ buffers on its first vacuum sweep.  On several x-slab domains
(comm.init) the step exchanges one neighbour layer of the five grids it reads, the sweep two
layers of the variables and one of fac_time (Comm.sendrecv), and the flag is reduced with
Comm.any; the kernels read those layers where one domain wraps around, so the result does not
depend on the number of domains, bit for bit.
"""
import ctypes
import itertools
import math
import types
import warnings

import torch

from .commons import is_selected, machine_ϵ, ρ_vacuum
from .lib import ConceptGPUError, _ptr, check, raw

_L = raw()

# The 8 triples of step/flux directions of the first MacCormack step (fluid.py:796-804): module
# state shared by all components, advanced once per maccormack() call.
STEP_TRIPLES = tuple(tuple(sign*s for s in triple) for sign in (+1, -1)
                     for triple in ((+1, +1, +1), (-1, +1, -1), (-1, -1, +1), (+1, -1, -1)))
_steps = itertools.cycle(STEP_TRIPLES)


def reset_steps():
    """Rewind the cycle of step triples to its first entry (tests)."""
    global _steps
    _steps = itertools.cycle(STEP_TRIPLES)


def _ptrs(tensors):
    """an array of the tensors' addresses; None stays None, like lib._ptr"""
    if tensors is None:
        return None
    return (ctypes.c_void_p*len(tensors))(*[t.data_ptr() for t in tensors])


def _halo_ptr(stack):
    """the address of the neighbour layers of a single grid, stack = lo or hi of
    _neighbour_layers(component, [grid], H); None (one domain) stays None"""
    return None if stack is None else _ptr(stack[0])


def _state(component):
    """the solver's buffers of a component, made at its first maccormack()"""
    st = component.__dict__.get('_maccormack_state')
    if st is None:
        z = lambda: torch.zeros_like(component.ϱ)
        st = types.SimpleNamespace(starred=[z(), z(), z(), z()], Δ=None, fac_time=z(),
                                   flag=torch.zeros(1, dtype=torch.int32, device=component.device))
        component._maccormack_state = st
    return st


def _ctx(component):
    # (the kernels use a context for its stream, launch checks and scratch memory only)
    return component._mesh()._ctx


def _grids(component):
    return [component.ϱ] + list(component.J)


def _neighbour_layers(component, tensors, H):
    """(lo, hi): the H layers below and above this domain's own of every tensor, stacked, from
    the neighbouring domains; (None, None) on one domain, where the kernels wrap around"""
    if component.nprocs == 1:
        return None, None
    if component.nxl < H:
        raise ConceptGPUError(f'{component.name}: {component.nxl} layers per domain, the fluid '
                              f'solver needs at least {H}')
    comm = component.comm
    up = torch.stack([t[-H:] for t in tensors]).contiguous()   # -> lo of the next domain
    down = torch.stack([t[:H] for t in tensors]).contiguous()  # -> hi of the previous domain
    lo, hi = torch.empty_like(up), torch.empty_like(down)
    comm.sendrecv(up, comm.next, lo, comm.prev)
    comm.sendrecv(down, comm.prev, hi, comm.next)
    return lo, hi


def _require_maccormack(component):
    """drift() and apply_internal_sources() are the MacCormack scheme and refuse any other"""
    scheme = is_selected(component, component.params.fluid_scheme_select)
    if scheme != 'maccormack':
        raise ConceptGPUError(
            f'{component.name}: fluid scheme "{scheme}" is not implemented (only "maccormack"; '
            'Kurganov-Tadmor is outside this path)')


def _check_closure_class(component):
    """what the shear term of closure 'class' (shear_sources) needs beyond _check_scope"""
    from . import ic
    name = component.name
    ic.check_shear_scope(component)
    if not component.approximations['P=wρ']:
        raise ConceptGPUError(
            f'{name}: Boltzmann closure "class" without the P=wρ approximation: the realisation '
            'of δ𝒫 with CLASS and the Hubble term of the continuity equation (fluid.py:1059-1067) '
            'are not implemented')
    scheme = is_selected(component, component.params.fluid_scheme_select)
    if scheme != 'maccormack':
        raise ConceptGPUError(
            f'{name}: Boltzmann closure "class" with the fluid scheme "{scheme}": the ς flux '
            'inside the limiter stage of Kurganov-Tadmor (fluid.py:425-460) is not implemented, '
            'only the source term of "maccormack"')


def _check_scope(component, a, closure_class=False):
    """closure_class: accept closure 'class' where the shear term is in scope (_check_closure_class);
    without it the closure is refused as it always was."""
    if component.representation != 'fluid':
        raise ConceptGPUError(f'{component.name}: the fluid solver was given a particle component')
    if closure_class and getattr(component, 'boltzmann_closure', 'truncate') == 'class':
        _check_closure_class(component)
    if component.boltzmann_order > 1:
        raise ConceptGPUError(
            f'{component.name}: boltzmann_order = {component.boltzmann_order}: the non-linear '
            'evolution of ς and 𝒫 (the shear term of maccormack_internal_sources) is not '
            'implemented')
    closure = getattr(component, 'boltzmann_closure', 'truncate')
    if closure != 'truncate' and not (closure_class and closure == 'class'):
        raise ConceptGPUError(
            f'{component.name}: Boltzmann closure "{closure}": realising ς with CLASS (the shear '
            'term of maccormack_internal_sources) is not implemented, only "truncate"')
    # a constant w (the reference's w_type 'constant'), for which w_eff = w at all times
    w_eff = component.w_eff(a=a)
    w = getattr(component, 'w_constant', 0.0)
    if getattr(component, 'w_type', 'constant') != 'constant' or w_eff != w:
        raise ConceptGPUError(
            f'{component.name}: w_eff = {w_eff} at a = {a} with the constant w = {w}: an equation '
            'of state that varies in time (w from CLASS, an expression or a table; decaying '
            'species) is not implemented')
    if w != 0 and not component.approximations['P=wρ']:
        # (unreachable through Component: species.py:1678-1685 forces the approximation on)
        raise ConceptGPUError(
            f'{component.name}: w = {w} without the P=wρ approximation: a non-linear 𝒫 and the '
            'Hubble term of the continuity equation (fluid.py:1059-1067) are not implemented')


def _c2w(component, a):
    return component.params.light_speed**2*component.w(a=a)


def realize_𝒫(component, a=1.0, closure_class=False):
    """realize_if_linear(2, 'trace') under the P=wρ approximation (realize_approximative,
    ic.py:495-509): 𝒫 = ϱ*(c²w)."""
    _check_scope(component, a, closure_class)
    check(_L.cg_fluid_pressure_sources(
        _ctx(component), _ptr(component.ϱ), None, None, _ptr(component.𝒫), None,
        component.gridsize, component.nxl, float(_c2w(component, a)), 0.0, 0.0))


def internal_sources(component, ᔑdt, a_next=-1, closure_class=False):
    """maccormack_internal_sources (fluid.py:990-1067) within scope: the pressure term of the
    Euler equation, ΔJⁱ = -ᔑa**(-3*w_eff)dt ∂ⁱ𝒫, with the order-2 difference of diff_domaingrid
    (mesh.py:4966-4970).  The reference reads the 𝒫 grid that kick_long realised just before
    (main.py:1133-1138); here the same pass realises it, 𝒫 = ϱ*(c²w), and forms the
    neighbours' values by the same product.  The shear term belongs to boltzmann_order > 1 or
    closure 'class' (refused), the Hubble term of the continuity equation to
    not approximations['P=wρ'], which species.py:1678-1685 rules out for this scope."""
    a = a_next if a_next != -1 else 1.0
    _check_scope(component, a, closure_class)
    p = component.params
    Δx = p.boxsize/component.gridsize
    lo, hi = _neighbour_layers(component, [component.ϱ], 1)
    check(_L.cg_fluid_pressure_sources(
        _ctx(component), _ptr(component.ϱ), _halo_ptr(lo), _halo_ptr(hi), _ptr(component.𝒫),
        _ptrs(list(component.J)), component.gridsize, component.nxl, float(_c2w(component, a)),
        float(-ᔑdt['a**(-3*w_eff)', component.name]), float((1/2)/Δx)))


def apply_internal_sources(component, ᔑdt, a_next=-1):
    """Component.apply_internal_sources (species.py:2812-2921) within scope; the `fluid_sources`
    hook of stepper.Timeloop.  Nothing happens for w = 0, exactly as the reference's condition
    (species.py:2886-2889) with the Hubble and shear terms out of scope.  The mom_decay_factor
    of species.py:2840-2865 is 1 for a_next = -1; otherwise the reference scales J by it only
    for components holding the CLASS species 'dcdm' — decaying species are out of scope, so it
    is never applied here."""
    if component.representation != 'fluid':
        return   # particle components have no special internal source terms
    _require_maccormack(component)
    _check_scope(component, a_next if a_next != -1 else 1.0)
    if component.boltzmann_order > 0 and not (component.w_type == 'constant'
                                              and component.w_constant == 0):
        internal_sources(component, ᔑdt, a_next)


def maccormack_step(component, ᔑdt, steps, mc_step, halve=False):
    """maccormack_step (fluid.py:841-946) and its ghost exchange (:951-960): the starred grids
    from the unstarred ones (mc_step 0) or the unstarred ones from the starred (mc_step 1)."""
    st = _state(component)
    p = component.params
    src, dst = (_grids(component), st.starred) if mc_step == 0 else (st.starred, _grids(component))
    src = src + [component.𝒫]
    Δx = p.boxsize/component.gridsize
    factor = -ᔑdt['a**(3*w_eff-2)', component.name]/Δx
    lo, hi = _neighbour_layers(component, src, 1)
    check(_L.cg_fluid_mc_step(
        _ctx(component), _ptrs(src), _ptrs(lo), _ptrs(hi), _ptrs(dst), component.gridsize,
        component.nxl, (ctypes.c_int*3)(*[int(s) for s in steps]), float(factor),
        float(p.light_speed**(-2)), int(mc_step), int(bool(halve))))


def _any(component, st):
    flag = bool(st.flag.item())
    if component.nprocs > 1:
        flag = component.comm.any(flag)
    return flag


def correct_vacuum(component, mc_step, record=None):
    """correct_vacuum (fluid.py:1157-1343): True if vacuum was imminent anywhere and one sweep of
    corrections was applied.  record: a list that receives (mc_step, fac_time of this domain's
    cells as a host array) for every sweep."""
    st = _state(component)
    mc = component.params.fluid_options['maccormack']
    foresight = is_selected(component, mc['foresight_select'])
    fac_smoothing = 1./(6 + 12./2. + 8./3.)*is_selected(component, mc['smoothing_select'])
    ctx = _ctx(component)
    n = component.ϱ.numel()
    # in the second step the starred and the unstarred variables swap roles (fluid.py:1229-1237)
    if mc_step == 0:
        a, b, var = component.ϱ, st.starred[0], _grids(component)
        k1, threshold = 2/foresight - 1, 2/foresight*ρ_vacuum
    else:
        a, b, var = st.starred[0], component.ϱ, st.starred
        k1, threshold = 0.0, 2*ρ_vacuum
    check(_L.cg_fluid_vacuum_detect(ctx, _ptr(a), _ptr(b), n, int(mc_step), float(k1),
                                    float(threshold), float(ρ_vacuum), _ptr(st.fac_time),
                                    _ptr(st.flag)))
    if not _any(component, st):
        return False
    if record is not None:
        record.append((mc_step, st.fac_time.cpu().numpy().copy()))
    if st.Δ is None:
        st.Δ = [torch.zeros_like(component.ϱ) for _ in range(4)]
    lo, hi = _neighbour_layers(component, var, 2)
    ft_lo, ft_hi = _neighbour_layers(component, [st.fac_time], 1)
    check(_L.cg_fluid_vacuum_gather(
        ctx, _ptrs(var), _ptrs(lo), _ptrs(hi), _ptr(st.fac_time), _halo_ptr(ft_lo),
        _halo_ptr(ft_hi), _ptrs(st.Δ), component.gridsize, component.nxl, float(fac_smoothing)))
    check(_L.cg_fluid_vacuum_apply(ctx, _ptrs(var), _ptrs(st.Δ), n))
    return True


def check_vacuum(component, mc_step):
    """check_vacuum (fluid.py:1079-1101): warn about densities below ρ_vacuum, correct nothing"""
    st = _state(component)
    ϱ = component.ϱ if mc_step == 0 else st.starred[0]
    check(_L.cg_fluid_vacuum_detect(_ctx(component), _ptr(ϱ), None, ϱ.numel(), 2, 0.0,
                                    float(ρ_vacuum), float(ρ_vacuum), None, _ptr(st.flag)))
    if _any(component, st):
        warnings.warn(f'Vacuum detected in {component.name}')


def finish(component, halve=True):
    """the epilogue of maccormack (fluid.py:784-792): both steps together leave double the
    values of all variables, and the starred and Δ buffers are left with no junk"""
    st = _state(component)
    check(_L.cg_fluid_mc_finish(_ctx(component), _ptrs(_grids(component)), _ptrs(st.starred),
                                _ptrs(st.Δ), component.ϱ.numel(), int(bool(halve))))


def maccormack(component, ᔑdt, a_next=-1, record=None, closure_class=False):
    """maccormack (fluid.py:724-792).  component.maccormack_attempts holds the number of
    attempts of the two steps of the last call, component.maccormack_sweeps the vacuum sweeps.
    closure_class: take a component of closure 'class' too (its flux terms are these; its shear
    term is a source, shear_sources)."""
    if component.boltzmann_order == 0:
        return   # no J variable: nothing to do (fluid.py:727-730)
    a = a_next if a_next != -1 else 1.0
    _check_scope(component, a, closure_class)
    # (a w = 0 component takes the path it always took: its 𝒫 grid is left as it is)
    pressure = getattr(component, 'w_constant', 0.0) != 0
    mc = component.params.fluid_options['maccormack']
    max_vacuum_corrections = [component.gridsize if v == 'gridsize' else v for v in
                              is_selected(component, mc['max_vacuum_corrections_select'])]
    correct = is_selected(component, mc['vacuum_corrections_select'])
    steps = list(next(_steps))
    attempts, sweeps = [0, 0], [0, 0]
    halved = False
    for mc_step in range(2):
        for attempt in range(max_vacuum_corrections[mc_step]):
            attempts[mc_step] += 1
            # the first step is re-evolved at each attempt, the second evolved once and then
            # corrected repeatedly
            if attempt == 0 or mc_step == 0:
                # a second step that no sweep can follow leaves the halved values at once
                halved = mc_step == 1 and not correct
                if mc_step == 0 and pressure:
                    # 𝒫 is re-realised from the unstarred ϱ before every first step
                    # (fluid.py:912-913) and used as it is in the second
                    realize_𝒫(component, a, closure_class=closure_class)
                maccormack_step(component, ᔑdt, steps, mc_step, halve=halved)
            if correct:
                if not correct_vacuum(component, mc_step, record):
                    break
                sweeps[mc_step] += 1
            else:
                check_vacuum(component, mc_step)
                break
        else:
            if mc_step == 1:
                component.maccormack_attempts, component.maccormack_sweeps = attempts, sweeps
                raise ConceptGPUError(
                    f'Giving up after {max_vacuum_corrections[mc_step]} failed attempts '
                    f'to remove negative densities in {component.name}')
        steps = [-s for s in steps]
    component.maccormack_attempts, component.maccormack_sweeps = attempts, sweeps
    finish(component, halve=not halved)


def drift(component, ᔑdt, a_end=-1, closure_class=False):
    """Component.drift for fluids (species.py:2200-2216); the `fluid_drift` hook of
    stepper.Timeloop.  closure_class: as for maccormack()."""
    if component.representation != 'fluid':
        raise ConceptGPUError(f'{component.name}: fluid.drift() is for fluid components')
    _require_maccormack(component)
    maccormack(component, ᔑdt, a_end, closure_class=closure_class)


# -- the Kurganov-Tadmor scheme --------------------------------------------------------------------
# flux_limiter_select -> the limiter id of cg_fluid_kt_step, with the reference's aliases
# (fluid.py:208-227)
FLUX_LIMITERS = {'minmod': 0, 'monotonizedcentral': 1, 'mc': 1, 'ospre': 2, 'superbee': 3,
                 'sweby': 4, 'umist': 5, 'vanalbada': 6, 'vanleer': 7, 'muscl': 7, 'harmonic': 7,
                 'koren': 8}


def _kt_options(component):
    return component.params.fluid_options['kurganovtadmor']


def kt_step_scale_factors(cosmo, a, Δt):
    """The scale factors of the two Runge-Kutta steps of order 2 under enable_Hubble
    (fluid.py:160-173): `a` belongs to the middle of the drift of duration Δt = ᔑdt['1'], the
    steps to the middles of its two halves.  cosmo: an integration.Cosmology with its clock
    initialised."""
    t_flux = cosmo.cosmic_time(a) - 0.5*Δt
    return cosmo.scale_factor(t_flux + 0.25*Δt), cosmo.scale_factor(t_flux + 0.75*Δt)


def kurganov_tadmor_step(component, ᔑdt, a, rk_order, rk_step, limiter):
    """One Runge-Kutta step of kurganov_tadmor (fluid.py:174-464) and its finalize_rk_step
    (:565-586): the starred grids from the unstarred ones (rk_step 0) or the update of the
    unstarred ones from the starred (rk_step 1).  The 𝒫 grid receives ϱ*(c²w) of the grids the
    step reads (realize_if_linear(2, 'trace', a, use_gridˣ), fluid.py:240; a linear 𝒫 has one
    buffer for both views, species.py:259-275).  `a` is the scale factor of this step, limiter
    an id of FLUX_LIMITERS."""
    st = _state(component)
    p = component.params
    name = component.name
    src, dst = (_grids(component), st.starred) if rk_step == 0 else (st.starred, _grids(component))
    Δx = p.boxsize/component.gridsize
    w = component.w(a=a)
    w_eff = component.w_eff(a=a)
    soundspeed = p.light_speed*math.sqrt(w)/a
    # (the pressure joins the flux only for w ≠ 0, use_𝒫 of fluid.py:316)
    f_𝒫 = ᔑdt['a**(-3*w_eff)', name]/ᔑdt['1'] if w != 0 else 0.0
    lo, hi = _neighbour_layers(component, src, 2)
    check(_L.cg_fluid_kt_step(
        _ctx(component), _ptrs(src), _ptrs(lo), _ptrs(hi), _ptrs(dst), _ptr(component.𝒫),
        component.gridsize, component.nxl, int(limiter), int(rk_step),
        float(p.light_speed**2*w), float(p.light_speed**(-2)), float(a**(3*w_eff - 2)),
        float(soundspeed), float(ᔑdt['a**(3*w_eff-2)', name]/ᔑdt['1']), float(f_𝒫),
        float((1 + rk_step)/rk_order*ᔑdt['1']/Δx)))


def kurganov_tadmor(component, ᔑdt, a, rk_order=2, cosmo=None):
    """kurganov_tadmor (fluid.py:103-464) with finalize_rk_step (:565-586): the flux terms of
    the continuity and Euler equations, the pressure term among them, by one (rk_order 1) or two
    Runge-Kutta steps.  a: the scale factor the reference takes from universals.a
    (species.py:2230).  cosmo: the integration.Cosmology that maps it onto the scale factors of
    the two steps (kt_step_scale_factors); needed for rk_order 2 under enable_Hubble.  There is no
    vacuum correction in this scheme."""
    if component.boltzmann_order < 1:
        return   # no J variable: nothing to do (fluid.py:139-142)
    if rk_order not in (1, 2):
        raise ConceptGPUError('Only Runge-Kutta orders 1 and 2 are implemented for the '
                              f'Kurganov-Tadmor method ({component.name}: {rk_order})')
    name = is_selected(component, _kt_options(component)['flux_limiter_select'])
    if name not in FLUX_LIMITERS:
        raise ConceptGPUError(f'Flux limiter "{name}" not implemented')
    _check_scope(component, a)
    a_steps = [a]*rk_order
    if component.params.enable_Hubble and rk_order == 2:
        if cosmo is None:
            raise ConceptGPUError(
                f'{component.name}: Kurganov-Tadmor of Runge-Kutta order 2 with enable_Hubble '
                'needs cosmo, the integration.Cosmology that gives the scale factors of its two '
                'steps')
        a_steps = kt_step_scale_factors(cosmo, a, ᔑdt['1'])
    for rk_step in range(rk_order):
        _check_scope(component, a_steps[rk_step])
        kurganov_tadmor_step(component, ᔑdt, a_steps[rk_step], rk_order, rk_step,
                             FLUX_LIMITERS[name])
    if rk_order == 1:
        # Euler integration: the updated grids are the starred ones (fluid.py:573-577)
        for grid, starred in zip(_grids(component), _state(component).starred):
            grid.copy_(starred)


def kurganov_tadmor_internal_sources(component, ᔑdt, a=-1):
    """The Kurganov-Tadmor branch of Component.apply_internal_sources (species.py:2902-2916):
    the flux step holds every term but the Hubble term of the continuity equation, which needs
    approximations['P=wρ'] off and is not implemented.  Within scope nothing happens."""
    _check_scope(component, a if a != -1 else 1.0)
    if (component.boltzmann_order > -1 and not component.approximations['P=wρ']
            and component.params.enable_Hubble):
        raise ConceptGPUError(
            f'{component.name}: the Hubble term of kurganov_tadmor_internal_sources '
            '(fluid.py:689-709, a non-linear 𝒫 without the P=wρ approximation) is not '
            'implemented')


def _clock(component):
    clock = component.__dict__.get('clock')
    if clock is None:
        raise ConceptGPUError(
            f'{component.name}: the Kurganov-Tadmor hook needs the clock of the time loop '
            '(component.clock, set by stepper.Timeloop) for the current scale factor')
    return clock


def drift_selected(component, ᔑdt, a_end=-1):
    """Component.drift for fluids (species.py:2200-2236) with both schemes; a `fluid_drift` hook
    of stepper.Timeloop.  'maccormack' goes to drift(); 'kurganovtadmor' to kurganov_tadmor()
    with the selected rungekuttaorder and, as the reference passes no scale factor
    (species.py:2230), the current one of the loop's clock: the start of the drift
    (main.py:335-361)."""
    if component.representation != 'fluid':
        raise ConceptGPUError(f'{component.name}: fluid.drift_selected() is for fluid components')
    if is_selected(component, component.params.fluid_scheme_select) != 'kurganovtadmor':
        return drift(component, ᔑdt, a_end)
    if component.boltzmann_order < 1:
        return
    clock = _clock(component)
    kurganov_tadmor(component, ᔑdt, clock.a,
                    rk_order=is_selected(component, _kt_options(component)['rungekuttaorder']),
                    cosmo=clock)


def sources_selected(component, ᔑdt, a_next=-1):
    """Component.apply_internal_sources (species.py:2812-2921) with both schemes; a
    `fluid_sources` hook of stepper.Timeloop."""
    if component.representation != 'fluid':
        return
    if is_selected(component, component.params.fluid_scheme_select) != 'kurganovtadmor':
        return apply_internal_sources(component, ᔑdt, a_next)
    kurganov_tadmor_internal_sources(component, ᔑdt, a_next)


def v_max(component, a, closure_class=False):
    """measure(component, 'v_max') for a fluid with non-linear J (analysis.py:3940-3963): the
    largest bulk velocity plus the sound speed light_speed*sqrt(w)/a.  The 𝒫 grid is read as it
    stands (realize_𝒫 or the last source pass filled it)."""
    _check_scope(component, a, closure_class)
    if component.boltzmann_order == 0:
        return 0.0
    p = component.params
    out = torch.zeros(1, dtype=torch.float64, device=component.device)
    check(_L.cg_fluid_vmax(_ctx(component), _ptr(component.ϱ), _ptr(component.𝒫),
                           _ptrs(list(component.J)), component.ϱ.numel(),
                           float(p.light_speed**(-2)), _ptr(out)))
    J_over_ϱ_plus_𝒫_2_max = float(out.item())
    if component.nprocs > 1:
        J_over_ϱ_plus_𝒫_2_max = float(
            component.comm.all_gather_floats([J_over_ϱ_plus_𝒫_2_max]).max())
    w_eff = component.w_eff(a=a)
    v = a**(3*w_eff - 2)*math.sqrt(J_over_ϱ_plus_𝒫_2_max)
    # the global sound speed (analysis.py:3956-3963); a w = 0 component returns what it did
    w = getattr(component, 'w_constant', 0.0)
    if w != 0:
        v += component.params.light_speed*math.sqrt(w)/a
    return v


def courant_limit(component, a, closure_class=False):
    """The Courant condition on the base step (main.py:803-823, fac_courant of main.py:2413);
    the `fluid_limiter` hook of stepper.Timeloop."""
    p = component.params
    fac_courant = 0.21*p.Δt_base_nonlinear_factor
    v = v_max(component, a, closure_class=closure_class)
    if v == 0:
        v = machine_ϵ   # a completely static component counts as just above 0
    return fac_courant*(p.boxsize/component.gridsize)/v


# -- closure 'class': the shear term of the Euler equation -----------------------------------------
def shear_sources(component, ᔑdt, amplitudes, a_next=-1, timings=None):
    """The shear term of maccormack_internal_sources (fluid.py:1011-1043) for a component of
    closure 'class' and boltzmann_order = 1: ΔJⁱ = -ᔑa**(-3*w_eff)dt ∂ʲςⁱⱼ, ς realised from the
    component's own ϱ (ic.fluid_structure) and the k²-indexed table `amplitudes` of σ
    (ic.amplitudes_from_transfer_ratio; the caller's transfer functions at a_next).

    The reference realises the six ςⁱⱼ, each with a backward transform, and differentiates them
    with the order-2 central difference.  On a periodic grid that difference along j is the
    factor i·sin(2π kⱼ/gridsize)/Δx in Fourier space, so the divergence is formed there
    (cg_shear_divergence): one forward transform of ϱ and three backward transforms, no ς grid.
    ς itself is ic.realize_shear().  timings: a dict that receives milliseconds by kind of pass
    (synchronises)."""
    from . import ic
    a = a_next if a_next != -1 else 1.0
    _check_scope(component, a, closure_class=True)
    if component.boltzmann_closure != 'class':
        raise ConceptGPUError(
            f'{component.name}: Boltzmann closure "{component.boltzmann_closure}" has no shear '
            'term: shear_sources() is for closure "class"')
    amplitudes_dev = ic._amplitudes_dev(component, amplitudes, component.gridsize,
                                        'a fluid grid of {}³ cells')
    # ς = ϱ_bar(1 + w)σ (ic.py:471-475) under the factor of the potential (fluid.py:1028)
    factor = -ᔑdt['a**(-3*w_eff)', component.name]*(component.ϱ_bar*(1 + component.w(a=a)))
    watch = ic._Stopwatch(timings)
    with watch('structure'):
        structure = ic.fluid_structure(component)
    work = ic._realization_mesh(component, 'realize work')
    for dim in range(3):
        with watch('k-space'):
            work.shear_divergence(structure, amplitudes_dev, dim)
        with watch('transforms'):
            work.poisson_backward()
        with watch('stores'):
            work.fluid_add_from_mesh(component.J[dim], factor)
    watch.finish()


def closure_sources(amplitudes_of):
    """A `fluid_sources` hook of stepper.Timeloop that knows closure 'class'.  For a component
    of that closure with boltzmann_order = 1 it calls amplitudes_of(component, a) for the
    k²-indexed table of σ at the scale factor of the kick's end, applies the shear term
    (shear_sources) and then the pressure term (internal_sources): the reference's order
    (fluid.py:1011-1058).  Every other component goes to sources_selected() unchanged."""
    def sources(component, ᔑdt, a_next=-1):
        if (component.representation != 'fluid'
                or getattr(component, 'boltzmann_closure', 'truncate') != 'class'):
            return sources_selected(component, ᔑdt, a_next)
        a = a_next if a_next != -1 else 1.0
        _check_scope(component, a, closure_class=True)
        shear_sources(component, ᔑdt, amplitudes_of(component, a), a_next)
        if not (component.w_type == 'constant' and component.w_constant == 0):
            internal_sources(component, ᔑdt, a_next, closure_class=True)
    return sources


def closure_hooks(amplitudes_of):
    """The three fluid hooks of stepper.Timeloop with closure 'class' in scope:
    Timeloop(components, **fluid.closure_hooks(amplitudes_of)).  Components of another closure
    take the paths of drift(), courant_limit() and sources_selected()."""
    import functools
    return {'fluid_drift': functools.partial(drift, closure_class=True),
            'fluid_limiter': functools.partial(courant_limit, closure_class=True),
            'fluid_sources': closure_sources(amplitudes_of)}
