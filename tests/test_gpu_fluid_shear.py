"""The shear of closure 'class' on the GPU (cg_realize_grid_tensor, cg_shear_divergence and
cg_fluid_add_from_mesh in csrc/cg_lpt.hip; ic.realize_shear, fluid.shear_sources,
fluid.closure_sources): each kernel against the plain numpy references of tests/shear_refs.py, the
divergence formed in Fourier space against the six-grid route of the reference, a plane wave in
closed form, momentum conservation, and the hook in the time loop.

Bars.  A pure k-space pass: 1e-14 of the largest value (the bar of test_gpu_fluid_ic.py); the
accumulating store rounds its product and its sum in turn: bit-identical.  Everything that goes
through the transforms: the project's 1e-12, of max |ς| or max |ΔJ|.  Every test prints what it
measured before it asserts."""
import numpy as np
import pytest

import lpt_refs
import shear_refs
from test_gpu_lpt import close, dev, meshes

pytestmark = pytest.mark.gpu
L = 100.0
W = 1/3
GRIDSIZES = [8, 12, 16]


def load(**more):
    from concept_amd import commons
    user = {'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25,
            'select_eos_w': {'nu': W}, 'select_approximations': {'all': {'P=wρ': True}},
            'select_boltzmann_closure': {'nu': 'class'},
            'realization_options': {'structure': {'nu': 'nonlinear'}}}
    user.update(more)
    return commons.load_params(user)


def neutrinos(ϱ, J=None):
    from test_gpu_fluid_drift import make_fluid
    g = ϱ.shape[0]
    c = make_fluid(ϱ, np.zeros((3, g, g, g)) if J is None else J, name='nu', species='neutrino')
    assert c.boltzmann_closure == 'class' and c.w_constant == W
    return c


def sdt(c, dt):
    return {'1': dt, ('a**(-3*w_eff)', c.name): dt}


def random_slab(g):
    """dense also where the kernels must write zeros"""
    return np.random.default_rng(g).normal(size=(g, g, g + 2))


def exactly_zero_where_dead(got, g):
    nyq = g//2
    return not (got[0, 0, :2].any() or got[nyq].any() or got[:, nyq].any()
                or got[:, :, 2*nyq:].any())


# ---- the k-space passes --------------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_realize_grid_tensor_against_numpy(gridsize):
    g = gridsize
    slab, table = random_slab(g), shear_refs.random_table(g, g)
    structure, out = meshes(g, 2)
    structure.upload_fourier(slab)
    for m in range(3):
        for n in range(3):
            out.upload_fourier(np.full_like(slab, 7.0))
            got = out.realize_grid_tensor(structure, dev(table), m, n).fetch_fourier()
            assert close(got, shear_refs.realize_grid_tensor(slab, table, m, n), 1e-14), (m, n)
            assert exactly_zero_where_dead(got, g)
    assert np.array_equal(structure.fetch_fourier(), slab)
    # in place
    structure.realize_grid_tensor(structure, dev(table), 1, 2)
    assert close(structure.fetch_fourier(), shear_refs.realize_grid_tensor(slab, table, 1, 2),
                 1e-14)


@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_shear_divergence_against_numpy(gridsize):
    g = gridsize
    slab, table = random_slab(g), shear_refs.random_table(g, g)
    structure, out = meshes(g, 2)
    structure.upload_fourier(slab)
    for dim in range(3):
        out.upload_fourier(np.full_like(slab, 7.0))
        got = out.shear_divergence(structure, dev(table), dim).fetch_fourier()
        assert close(got, shear_refs.shear_divergence(slab, table, dim, L), 1e-14), dim
        assert exactly_zero_where_dead(got, g)
    assert np.array_equal(structure.fetch_fourier(), slab)


def test_the_k_space_refusals():
    from concept_amd.lib import ConceptGPUError
    a, b = meshes(8, 2)
    c, = meshes(12, 1)
    for call in (lambda *args: a.realize_grid_tensor(*args, 0, 0),
                 lambda *args: a.shear_divergence(*args, 0)):
        with pytest.raises(ConceptGPUError, match=r'27 amplitudes for grid size 8, which needs '
                                                  r'3\*\(nyquist - 1\)\*\*2 \+ 1 = 28'):
            call(b, dev(np.zeros(27)))
        with pytest.raises(ConceptGPUError, match='differ in grid size or domain'):
            call(c, dev(np.zeros(28)))
    with pytest.raises(ConceptGPUError, match=r'indices \(0, 3\) not in \{0, 1, 2\}'):
        a.realize_grid_tensor(b, dev(np.zeros(28)), 0, 3)
    with pytest.raises(ConceptGPUError, match=r'dim = 3 not in \{0, 1, 2\}'):
        a.shear_divergence(b, dev(np.zeros(28)), 3)
    # the old entry still refuses rank 2
    with pytest.raises(ConceptGPUError, match=r'tensor rank 2 \(0 and 1 are implemented\)'):
        a.realize_grid(b, dev(np.zeros(28)), 2)


@pytest.mark.parametrize('gridsize', [12, 16])
def test_fluid_add_from_mesh_is_bit_identical(gridsize):
    """the mesh's padding (and the unused row of a layer at 16) is NaN: never read"""
    import torch
    rng = np.random.default_rng(gridsize)
    g = gridsize
    mesh, = meshes(g, 1)
    rows = mesh.layer_doubles//mesh.pad
    field, J = rng.normal(size=(g, g, g)), rng.normal(size=(g, g, g))
    native = np.full((g, rows, mesh.pad), np.nan)
    native[:, :g, :g] = field
    mesh.layers_write(0, g, dev(native))
    out = dev(J)
    for factor in (-0.37, 1.0):
        J = J + factor*field
        mesh.fluid_add_from_mesh(out, factor)
        assert np.array_equal(out.cpu().numpy(), J), factor
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError, match='fluid grids must be contiguous float64 tensors'):
        mesh.fluid_add_from_mesh(torch.zeros((g, g, g - 1), dtype=torch.float64, device='cuda'),
                                 1.0)


# ---- ς and its term of the Euler equation ---------------------------------------------------------
def shear_grids(c, a, table):
    """the six ςₘₙ through ic.realize_shear from one transform of ϱ, as host arrays"""
    from concept_amd import ic
    structure = ic.fluid_structure(c)
    return {(m, n): ic.realize_shear(c, a, table, (m, n), structure=structure).cpu().numpy()
            for m, n in shear_refs.PAIRS}


@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_realize_shear_is_traceless_repeatable_and_numpys(gridsize):
    import torch
    from concept_amd import ic
    load()
    g, a = gridsize, 0.5
    ϱ = shear_refs.random_density(g, g)
    table = shear_refs.random_table(g, g)
    c = neutrinos(ϱ)
    ς = shear_grids(c, a, table)
    scale = max(np.abs(v).max() for v in ς.values())
    trace = np.abs(ς[0, 0] + ς[1, 1] + ς[2, 2]).max()
    print(f'g = {g}: max |ς| = {scale:.3e}, max |ς₀₀ + ς₁₁ + ς₂₂| = {trace/scale:.3e} of it')
    assert scale > 0 and trace <= 1e-12*scale
    c0 = c.ϱ_bar*(1 + W)
    for (m, n), got in ς.items():
        err = np.abs(got - shear_refs.realize_shear(ϱ, table, m, n, c0)).max()
        print(f'ς[{m}{n}] within {err/scale:.3e} of max |ς| of numpy')
        assert err <= 1e-12*scale
    # the same bits again, in either order of the indices and into a tensor of the caller's
    out = torch.full((g, g, g), np.nan, dtype=torch.float64, device='cuda')
    assert ic.realize_shear(c, a, table, (2, 1), out=out) is out
    assert np.array_equal(out.cpu().numpy(), ς[1, 2])
    assert np.array_equal(ic.realize_shear(c, a, table, (1, 2)).cpu().numpy(), ς[1, 2])
    assert np.array_equal(c.host('ϱ'), ϱ) and not c.host('J').any()


@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_shear_sources_equals_the_six_grid_route_and_conserves_momentum(gridsize):
    from concept_amd import fluid
    load()
    g, a, dt = gridsize, 0.5, 0.037
    ϱ = shear_refs.random_density(g, g)
    table = shear_refs.random_table(g, g)
    J0 = np.random.default_rng(g).normal(size=(3, g, g, g))
    c = neutrinos(ϱ, J0)
    # realize_shear six times, the numpy central difference, J += -ᔑdt·…
    six = shear_refs.shear_sources_six(ϱ, J0, table, dt, None, L, ς=shear_grids(c, a, table))
    fluid.shear_sources(c, sdt(c, dt), table, a)
    J = c.host('J')
    ΔJ = six - J0
    scale = np.abs(ΔJ).max()
    err = np.abs(J - six).max()
    print(f'g = {g}: max |ΔJ| = {scale:.3e}; shear_sources within {err/scale:.3e} of it of the '
          'six-grid route')
    assert scale > 1e-3*np.abs(J0).max() and err <= 1e-12*scale
    assert np.array_equal(c.host('ϱ'), ϱ)
    # the increment alone, on J = 0: a divergence moves no net momentum
    c = neutrinos(ϱ)
    fluid.shear_sources(c, sdt(c, dt), table, a)
    ΔJ = c.host('J')
    for i in range(3):
        total, absolute = abs(ΔJ[i].sum()), np.abs(ΔJ[i]).sum()
        print(f'Σ ΔJ[{i}] = {total/absolute:.3e} of Σ |ΔJ[{i}]|')
        assert absolute > 0 and total <= 1e-13*absolute


@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_a_plane_wave_in_closed_form(gridsize):
    """ϱ = ϱ_bar(1 + ε cos φ), φ = 2π n⃗·x⃗/L with n⃗ = (1, 2, 0), and a constant ratio R.  ℱ[ϱ] is
    ϱ_bar ε g³/2 in the modes ±n⃗, the table R g⁻³/ϱ_bar, so σₘₙ = R ε Kₘₙ(n⃗) cos φ and
    ςₘₙ = ϱ_bar(1 + w)σₘₙ.  The central difference of cos φ along j is -(sin(2π nⱼ/g)/Δx) sin φ:
    ΔJⁱ = -ᔑdt ∂ʲςⁱⱼ = +ᔑdt ϱ_bar(1 + w) R ε (Σⱼ Kᵢⱼ(n⃗) sin(2π nⱼ/g)/Δx) sin φ."""
    from concept_amd import fluid, ic
    load()
    g, a, dt = gridsize, 0.5, 0.037
    n, ε, R, ϱ_bar = (1, 2, 0), 0.05, -0.8, 2.5
    x = np.arange(g)
    φ = 2*np.pi/g*(n[0]*x[:, None, None] + n[1]*x[None, :, None] + n[2]*x[None, None, :])
    c = neutrinos(ϱ_bar*(1 + ε*np.cos(φ)))
    assert c.ϱ_bar == pytest.approx(ϱ_bar, rel=1e-14)
    k = np.geomspace(0.5, 4*g, 7)*(2*np.pi/L)
    table = ic.amplitudes_from_transfer_ratio(k, np.full(k.size, R), g, L, ϱ_bar)
    fluid.shear_sources(c, sdt(c, dt), table, a)
    J = c.host('J')
    n2, Δx = sum(q*q for q in n), L/g
    s = [np.sin(2*np.pi*q/g)/Δx for q in n]
    S = [sum((0.5*(i == j) - 1.5*n[i]*n[j]/n2)*s[j] for j in range(3)) for i in range(3)]
    amplitude = abs(dt*ϱ_bar*(1 + W)*R*ε)*max(abs(v) for v in S)
    assert S[2] == 0 and min(abs(S[0]), abs(S[1])) > 0
    for i in range(3):
        err = np.abs(J[i] - dt*ϱ_bar*(1 + W)*R*ε*S[i]*np.sin(φ)).max()
        print(f'g = {g}: ΔJ[{i}] within {err/amplitude:.3e} of the amplitude {amplitude:.3e}')
        assert err <= 1e-12*amplitude


def test_against_the_golden_of_the_reference(golden):
    """the reference's own realize_grid of rank 2 and diff_domaingrid of order 2 on g = 8
    (tests/golden/fluid_shear_g8.npz): ςₘₙ of realize_shear and ΔJ of shear_sources, 1e-12"""
    from concept_amd import fluid
    from test_shear_refs_host import golden_increment
    g = golden('fluid_shear_g8')
    load(boxsize=float(g['boxsize']))
    a, dt = float(g['a']), 0.037
    c = neutrinos(g['rho'])
    c0 = c.ϱ_bar*(1 + W)
    ς = shear_grids(c, a, g['amplitudes'])
    for (m, n), got in ς.items():
        want = c0*g[f'sigma_{m}{n}']
        err = np.abs(got - want).max()/np.abs(want).max()
        print(f'ς[{m}{n}] within {err:.3e} of the golden\'s largest value')
        assert err <= 1e-12
    fluid.shear_sources(c, sdt(c, dt), g['amplitudes'], a)
    want = golden_increment(g, dt, c0)
    err = np.abs(c.host('J') - want).max()/np.abs(want).max()
    print(f'ΔJ within {err:.3e} of max |ΔJ| of the golden\'s route')
    assert err <= 1e-12


# ---- the hook in the time loop --------------------------------------------------------------------
def run_loop(closure, table):
    """a w = 1/3 fluid under its own gravity on grid size 12 (and particles that feel no force)
    for a few base steps; closure 'class' with the hooks of fluid.closure_hooks"""
    from concept_amd import commons, fluid, stepper
    from concept_amd.species import Component
    g = 12
    p = commons.load_params(
        "boxsize = 8.0*Mpc\npotential_options = {'gridsize': {'gravity': {'pm': 12}}}\n"
        "H0 = 70*km/s/Mpc\nΩcdm = 0.25\nΩb = 0.05\na_begin = 0.8\n"
        "select_forces = {'nu': {'gravity': 'pm'}}\nselect_eos_w = {'nu': 1/3}\n"
        "select_approximations = {'all': {'P=wρ': True}}\n"
        f"select_boltzmann_closure = {{'nu': '{closure}'}}\n"
        "realization_options = {'structure': {'nu': 'nonlinear'}}\n"
        "output_times = {'a': (0.8002,)}\noutput_dirs = {}\n")
    rng = np.random.default_rng(8)
    part = Component('matter', 'matter', N=64, mass=1.0)
    part.populate(rng.uniform(0, 8.0, (64, 3)), 'pos')
    part.populate(np.zeros((64, 3)), 'mom')
    q = (np.arange(g) + 0.5)*(2*np.pi/g)
    x, y, z = np.meshgrid(q, q, q, indexing='ij')
    ϱ = p.ρ_mbar*(1 + 0.2*np.sin(x)*np.cos(y) + 0.1*np.sin(z + y))
    from test_gpu_fluid_drift import make_fluid
    fl = make_fluid(ϱ, np.zeros((3, g, g, g)), name='nu', species='neutrino')
    assert fl.boltzmann_closure == closure
    asked = []
    if closure == 'class':
        def amplitudes_of(component, a):
            asked.append((component.name, a))
            return table(component, p)
        hooks = fluid.closure_hooks(amplitudes_of)
    else:
        hooks = dict(fluid_drift=fluid.drift, fluid_limiter=fluid.courant_limit,
                     fluid_sources=fluid.apply_internal_sources)
    fluid.reset_steps()
    loop = stepper.Timeloop([part, fl], **hooks)
    loop.run()
    fluid.reset_steps()
    return ϱ, fl.host('ϱ'), fl.host('J'), len(loop.history), asked


def test_timeloop_with_the_closure_hook():
    """an all-zero table leaves the bits of the 'truncate' run; a table of the size of the
    pressure (σ ~ -c²w δ/10) changes J and leaves Σϱ alone (1e-13, the bar of the drift's own
    time-loop tests)"""
    k2_max = 3*(12//2 - 1)**2
    ϱ0, ϱ_t, J_t, steps_t, _ = run_loop('truncate', None)
    ϱ0, ϱ_z, J_z, steps_z, asked = run_loop('class', lambda c, p: np.zeros(k2_max + 1))
    print(f'{steps_t} base steps; the table was asked for {len(asked)} times')
    assert steps_t >= 3 and steps_z == steps_t
    assert len(asked) >= steps_t and all(name == 'nu' and 0.8 < a <= 0.8002 + 1e-12
                                         for name, a in asked)
    assert np.abs(J_t).max() > 0 and not np.array_equal(ϱ_t, ϱ0)
    assert np.array_equal(ϱ_z, ϱ_t) and np.array_equal(J_z, J_t)

    def table(c, p):
        out = np.full(k2_max + 1, -0.1*p.light_speed**2*W*12.0**(-3)/c.ϱ_bar)
        out[0] = 0
        return out
    ϱ0, ϱ_s, J_s, steps_s, _ = run_loop('class', table)
    change = np.abs(J_s - J_t).max()/np.abs(J_t).max()
    drift = abs(ϱ_s.sum() - ϱ0.sum())/ϱ0.sum()
    print(f'{steps_s} base steps with the shear term: J differs by {change:.3e} of max |J|, '
          f'Σϱ by {drift:.3e}')
    assert np.isfinite(J_s).all() and np.isfinite(ϱ_s).all() and ϱ_s.min() > 0
    assert change > 1e-3 and drift <= 1e-13
