"""3LPT and Orszag dealiasing on the GPU (cg_lpt_diff_enlarge, cg_lpt_dealias_cube and
cg_lpt_shrink_accumulate in csrc/cg_lpt.hip; LptTerms and realize_particles(extended=True) in
concept_amd/ic.py): each kernel against the plain numpy references of tests/lpt3_refs.py and
against the unfused passes it replaces, known answers of plane waves, the whole realisation
against the reference's own (tests/golden/lpt3_*.npz), and the hand-over to the time loop.

Bars.  The three kernels evaluate the reference's expressions in the reference's order and may
differ from numpy only through cos / sin of the size-change phase (a few ulp): 1e-14 of the
largest value.  Everything that goes through the transforms: the project's 1e-12 (README) — of a
cell for positions, of max |mom| for momenta, of its own largest magnitude for a potential.  The
round trip through both transforms of size M: 1e-13 of the derivative's scale."""
import glob
import os

import numpy as np
import pytest

import lpt3_refs
import lpt_refs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, 'lpt3_*.npz')))
L = 100.0
# (N, M): the +1 branch of M (10 -> 16), the hand-written transform (8, 16) and the library's
# (10, 12, 18, 24) on either side; at 256 threads a workgroup these are 2 (N = 8) to 28 (M = 24)
# workgroups, the last one partial
SIZES = [(8, 12), (12, 18), (10, 16), (16, 24)]
DIMS = [(i, -1) for i in range(3)] + [(i, j) for i in range(3) for j in range(i, 3)]


def meshes(g, n, boxsize=L):
    from concept_amd.mesh import PotentialMesh
    return [PotentialMesh(g, boxsize) for _ in range(n)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, ref, bar, what=''):
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f'{what} max error {err:.3e} = {err/scale:.3e} of the scale {scale:.3e} (bar {bar:.0e})')
    return err <= bar*scale


def test_the_sizes_are_the_dealiasing_sizes():
    from concept_amd import ic
    assert [(n, ic.dealias_gridsize(n)) for n, _ in SIZES] == SIZES


# ---- cg_lpt_diff_enlarge ---------------------------------------------------------------------
@pytest.mark.parametrize('n,m', SIZES)
def test_diff_enlarge_against_numpy_and_the_unfused_passes(n, m):
    """the source dense random, its Nyquist planes and origin included; the target pre-filled
    with a sentinel, so that a mode left unwritten shows"""
    rng = np.random.default_rng(n)
    slab = rng.normal(size=(n, n, n + 2))
    src, tmp = meshes(n, 2)
    dst, unfused = meshes(m, 2)
    src.upload_fourier(slab)
    outside = ~np.repeat(lpt3_refs.cube(n, m), 2, axis=2)
    for dim0, dim1 in DIMS:
        for factor in (1.0, -0.37):
            dst.upload_fourier(np.full((m, m, m + 2), 7.0))
            dst.lpt_diff_enlarge(src, dim0, dim1, factor)
            got = dst.fetch_fourier()
            assert not (got == 7.0).any(), (dim0, dim1, factor)
            assert not got[outside].any() and not got[0, 0, :2].any()
            ref = lpt3_refs.diff_enlarge(slab, m, dim0, dim1, factor, L)
            assert close(got, ref, 1e-14, f'({dim0}, {dim1}) x {factor} numpy:')
            tmp.lpt_diff(src, dim0, dim1, factor)
            unfused.upload_fourier(np.full((m, m, m + 2), 7.0))
            unfused.copy_modes_from(tmp)
            assert close(got, unfused.fetch_fourier(), 1e-14, 'unfused:')
    assert np.array_equal(src.fetch_fourier(), slab)


# ---- cg_lpt_dealias_cube -----------------------------------------------------------------------
@pytest.mark.parametrize('n,m', SIZES)
def test_dealias_cube_keeps_the_cube_bit_for_bit_and_zeroes_the_rest(n, m):
    rng = np.random.default_rng(m)
    slab = rng.normal(size=(m, m, m + 2))
    mesh, = meshes(m, 1)
    for n_small in (n, 2, m - 2):
        mesh.upload_fourier(slab)
        mesh.lpt_dealias_cube(n_small)
        got = mesh.fetch_fourier()
        inside = np.repeat(lpt3_refs.cube(n_small, m), 2, axis=2)
        assert np.array_equal(got[inside], slab[inside])
        assert not got[~inside].any()
        assert not got[lpt3_refs.nyquist_planes(m)].any()
        assert np.array_equal(got, lpt3_refs.dealias_cube(slab, n_small))
        assert inside.sum() == 2*(n_small - 1)**2*(n_small//2)


# ---- cg_lpt_shrink_accumulate ------------------------------------------------------------------
@pytest.mark.parametrize('n,m', SIZES)
def test_shrink_accumulate_ops_factors_and_nyquist_planes(n, m):
    rng = np.random.default_rng(n + m)
    slab = rng.normal(size=(m, m, m + 2))
    before = rng.normal(size=(n, n, n + 2))
    out, = meshes(n, 1)
    src, = meshes(m, 1)
    src.upload_fourier(slab)
    planes = lpt3_refs.nyquist_planes(n)
    for operation in ('=', '+=', '-='):
        for factor in (1.0, -0.5):
            out.upload_fourier(before)
            out.lpt_shrink_accumulate(src, operation, factor)
            got = out.fetch_fourier()
            ref = lpt3_refs.shrink_accumulate(before, slab, operation, factor)
            assert close(got, ref, 1e-14, f'{operation} x {factor}:')
            if operation == '=':
                assert not got[planes].any()
            else:
                assert np.array_equal(got[planes], before[planes])
    assert np.array_equal(src.fetch_fourier(), slab)
    # against the unfused passes: copy with phase into a nullified slab
    unfused, = meshes(n, 1)
    unfused.upload_fourier(before)
    unfused.copy_modes_from(src)
    out.lpt_shrink_accumulate(src, '=')
    assert close(out.fetch_fourier(), unfused.fetch_fourier(), 1e-14, 'unfused:')


@pytest.mark.parametrize('n,m', SIZES)
def test_round_trip_gives_back_the_derivative(n, m):
    """enlarge, inverse transform, forward transform, shrink with M⁻³"""
    rng = np.random.default_rng(3*n)
    slab = lpt_refs.to_fourier(rng.normal(size=(n, n, n)))
    src, out = meshes(n, 2)
    big, = meshes(m, 1)
    src.upload_fourier(slab)
    for dim0, dim1 in ((1, -1), (0, 2)):
        big.lpt_diff_enlarge(src, dim0, dim1)
        big.poisson_backward()
        big.fft_forward()
        out.lpt_shrink_accumulate(big, '=', float(m)**-3)
        assert close(out.fetch_fourier(), lpt_refs.diff(slab, dim0, dim1, 1.0, L), 1e-13)


def test_the_entry_points_refuse_by_name():
    from concept_amd.lib import ConceptGPUError
    small, = meshes(8, 1)
    big, = meshes(12, 1)
    other, = meshes(12, 1, boxsize=50.0)
    with pytest.raises(ConceptGPUError, match='cg_lpt_diff_enlarge: grid size 8 is not larger '
                                              'than 12'):
        small.lpt_diff_enlarge(big, 0)
    with pytest.raises(ConceptGPUError, match='cg_lpt_diff_enlarge: grid size 12 is not larger '
                                              'than 12'):
        big.lpt_diff_enlarge(big, 0)
    with pytest.raises(ConceptGPUError, match=r'dimensions \(0, 3\) outside 0..2'):
        big.lpt_diff_enlarge(small, 0, 3)
    with pytest.raises(ConceptGPUError, match=r'dimensions \(-1, -1\) outside 0..2'):
        big.lpt_diff_enlarge(small, -1)
    with pytest.raises(ConceptGPUError, match='cg_lpt_diff_enlarge: the two meshes span '
                                              'different boxes'):
        other.lpt_diff_enlarge(small, 0)
    with pytest.raises(ConceptGPUError, match='cg_lpt_shrink_accumulate: grid size 8 is not '
                                              'larger than 12'):
        big.lpt_shrink_accumulate(small)
    with pytest.raises(ConceptGPUError, match='cg_lpt_shrink_accumulate: the two meshes span'):
        small.lpt_shrink_accumulate(other)
    from concept_amd import lib
    with pytest.raises(ConceptGPUError, match='cg_lpt_shrink_accumulate: operation 3 not in'):
        lib.check(lib.raw().cg_lpt_shrink_accumulate(small._ctx, big._ctx, 3, 1.0))
    with pytest.raises(ConceptGPUError, match='cg_lpt_dealias_cube: grid size 12 is not larger '
                                              'than 12'):
        big.lpt_dealias_cube(12)
    with pytest.raises(ConceptGPUError, match='cg_lpt_dealias_cube: grid sizes 7 and 12 are not '
                                              'both even'):
        big.lpt_dealias_cube(7)
    with pytest.raises(ConceptGPUError, match='null context'):
        lib.check(lib.raw().cg_lpt_dealias_cube(None, 8))


# ---- known answers, independent of the reference --------------------------------------------------
NAMES = ('Φ2', 'Φ3a', 'Φ3b', 'A3c0', 'A3c1', 'A3c2')


def potentials_of(g, waves, dealias):
    """Φ⁽¹⁾ = ∇⁻²(δ) of plane waves with unit amplitudes, then every potential above it through
    LptTerms and carryout_lpt with all growth factors 1; real-space fields on the grid points"""
    import torch
    from concept_amd import ic
    Φ1, Φ2, Φ3, t0, t1 = meshes(g, 5)
    big = meshes(ic.dealias_gridsize(g), 2) if dealias else None
    slab = np.zeros((g, g, g + 2))
    for (ki, kj, kk), A in waves:
        assert kk > 0 or (ki, kj) > (0, 0)
        slab[kj % g, ki % g, 2*kk] = A
        if kk == 0:
            slab[-kj % g, -ki % g, 0] = A
    t0.upload_fourier(slab)
    Φ1.lpt_potential(t0, dev(np.ones(3*(g//2 - 1)**2 + 1)), factor=-1)
    live = np.repeat(lpt_refs.alive(g), 2, axis=2)
    fields = {'Φ1': lpt_refs.to_real(Φ1.fetch_fourier())}
    growth = {key: 1.0 for key in ic.GROWTH_FACTOR_KEYS}
    pos = torch.zeros((g**3, 3), dtype=torch.float64, device='cuda')
    mom = torch.zeros_like(pos)
    terms = ic.LptTerms({'Φ1': Φ1, 'Φ2': Φ2, 'Φ3': Φ3}, (t0, t1), big)
    ic.carryout_lpt(ic.lpt_orders(3), terms, growth, 0.02, 1.0, 1.0, (pos, mom, 0),
                    lambda name, mesh, factor: fields.__setitem__(
                        name, lpt_refs.to_real(mesh.fetch_fourier()*live)))
    assert set(fields) == set(NAMES) | {'Φ1'}
    return fields


@pytest.mark.parametrize('dealias', [False, True])
def test_a_single_plane_wave_has_no_higher_order_potential(dealias):
    g = 12
    fields = potentials_of(g, [((2, 1, 3), 0.8)], dealias)
    scale = np.abs(fields['Φ1']).max()
    assert scale == pytest.approx(2*0.8/(14*(2*np.pi/L)**2), rel=1e-12)
    # δ = 1.6 cos(k⃗·x⃗): every term of a source is of the size of Φ⁽¹⁾ times a power of δ's 1.6
    for name in NAMES:
        print(name, np.abs(fields[name]).max()/scale)
        assert np.abs(fields[name]).max() <= 1e-12*scale


WAVES_BEYOND = [((4, 0, 0), 0.8), ((3, 2, 0), -0.3)]  # the sum (7, 2, 0): beyond 6, inside 9


def test_two_crossed_waves_whose_sum_lies_beyond_nyquist():
    """N = 12, M = 18.  Dealiased, Φ⁽²⁾ holds the difference mode (1, -2, 0) alone, in closed
    form; un-dealiased, it also holds the sum mode where the grid sees it, at (-5, 2, 0), with the
    size that ∇⁻² gives it there."""
    g = 12
    ref1 = lpt3_refs.plane_waves(g, L, WAVES_BEYOND)
    scale = np.abs(ref1).max()
    dealiased = potentials_of(g, WAVES_BEYOND, True)
    assert np.abs(dealiased['Φ1'] - ref1).max() <= 1e-12*scale
    ref2 = lpt3_refs.phi2_of_two_waves(g, L, WAVES_BEYOND, keep_sum=False)
    err = np.abs(dealiased['Φ2'] - ref2).max()
    print(f'dealiased Φ2 within {err/scale:.3e} of the Φ1 scale, max |Φ2| {np.abs(ref2).max()/scale:.3e}')
    assert err <= 1e-12*scale and np.abs(ref2).max() > 1e-3*scale
    plain = potentials_of(g, WAVES_BEYOND, False)
    ref2_alias = lpt3_refs.phi2_of_two_waves(g, L, WAVES_BEYOND, alias_to=g)
    err = np.abs(plain['Φ2'] - ref2_alias).max()
    alias = np.abs(ref2_alias - ref2).max()
    print(f'plain Φ2 within {err/scale:.3e} of the Φ1 scale, the alias {alias/scale:.3e} of it')
    assert err <= 1e-12*scale
    # the alias is the sum mode's strength over |(-5, 2, 0)|² = 29 against |(1, -2, 0)|² = 5
    assert alias == pytest.approx(np.abs(ref2).max()*5/29, rel=1e-12)
    assert np.abs(plain['Φ2'] - dealiased['Φ2']).max() == pytest.approx(alias, rel=1e-9)


def test_two_crossed_waves_with_no_product_beyond_nyquist():
    """N = 16: every product of up to three of the waves (1, 2, 0) and (2, -1, 1) stays inside
    |k| < 8, so dealiasing changes nothing.  The bar is 1e-12 of the largest potential of the
    order: the third-order ones are of one unit, and Φ⁽³ᵃ⁾ of two waves vanishes by cancellation
    among terms of that size."""
    g = 16
    waves = [((1, 2, 0), 0.8), ((2, -1, 1), -0.3)]
    plain, dealiased = potentials_of(g, waves, False), potentials_of(g, waves, True)
    scales = {'Φ2': np.abs(plain['Φ2']).max()}
    scales.update({name: max(np.abs(plain[n]).max() for n in NAMES[1:]) for name in NAMES[1:]})
    ref2 = lpt3_refs.phi2_of_two_waves(g, L, waves)
    assert np.abs(plain['Φ2'] - ref2).max() <= 1e-12*np.abs(plain['Φ1']).max()
    for name in NAMES:
        err = np.abs(plain[name] - dealiased[name]).max()
        print(f'{name}: {err/scales[name]:.3e} of {scales[name]:.3e}, '
              f'own size {np.abs(plain[name]).max():.3e}')
        assert err <= 1e-12*scales[name]
    for name in ('Φ2', 'Φ3b', 'A3c0', 'A3c1', 'A3c2'):
        assert np.abs(plain[name]).max() > 1e-3*scales[name], name


# ---- end to end --------------------------------------------------------------------------------------
def realize(g):
    from concept_amd import commons, ic
    from concept_amd.species import Component
    commons.load_params(str(g['param_text']))
    n = int(g['gridsize'])
    c = Component('matter', 'matter', N=n**3, mass=float(g['mass']))
    ic.n_particles_realized.update(components_tally=int(g['components_tally']),
                                   components_total=int(g['components_total']),
                                   particles_tally=int(g['id_bgn']))
    growth = dict(zip(g['growth_keys'].tolist(), g['growth_values'].tolist()))
    potentials = {}
    grids = ic.realize_particles(
        c, float(g['a']), g['amplitudes'], g['amplitudes_θ'], growth, extended=True,
        on_potential=lambda name, mesh, factor: potentials.__setitem__(
            name, (factor, mesh.fetch_fourier())))
    return c, grids, potentials


@pytest.mark.parametrize('case', CASES)
def test_realize_particles_against_the_golden(golden, case):
    from concept_amd import ic
    g = golden('lpt3_' + case)
    n = int(g['gridsize'])
    c, grids, potentials = realize(g)
    pos, mom, ids = c.host('pos'), c.host('mom'), c.host('ids')
    assert np.array_equal(ids, g['ids'])
    d = np.abs(pos - g['pos'])
    d = np.minimum(d, L - d).max()/(L/n)
    e = np.abs(mom - g['mom']).max()/np.abs(g['mom']).max()
    print(f'{case}: positions within {d:.3e} of a cell, momenta within {e:.3e} of max |mom|')
    assert (pos >= 0).all() and (pos < L).all()
    assert ic.n_particles_realized['particles_tally'] == int(g['id_bgn']) + n**3
    dealias = 'dealias' in case
    assert grids['gridsize_dealias'] == (ic.dealias_gridsize(n) if dealias else n)
    # every potential the reference had after laplacian_inverse, off the planes nothing reads
    live = np.repeat(lpt_refs.alive(n), 2, axis=2)
    keys = {'Φ2': 'Phi2', 'Φ3a': 'Phi3a', 'Φ3b': 'Phi3b', 'A3c0': 'A3c0', 'A3c1': 'A3c1',
            'A3c2': 'A3c2'}
    expected = [name for name, key in keys.items() if key in g.files]
    assert list(potentials) == expected and len(expected) == (6 if '3lpt' in case else 1)
    worst = 0.0
    assert close(grids['Φ1'].fetch_fourier()*live, g['Phi1']*live, 1e-12, 'Φ1:')
    for name in expected:
        factor, got = potentials[name]
        assert factor == float(g[keys[name] + '_factor'])
        ref = g[keys[name]]*live
        err = np.abs(got*live - ref).max()/np.abs(ref).max()
        print(f'{name} within {err:.3e} of its own largest magnitude')
        worst = max(worst, err)
    assert worst <= 1e-12
    assert d <= 1e-12 and e <= 1e-12
    # a second run gives the same bits
    c2, _, _ = realize(g)
    assert np.array_equal(c2.host('pos'), pos) and np.array_equal(c2.host('mom'), mom)


def test_without_the_keyword_the_scope_is_refused_on_the_gpu_too(golden):
    from concept_amd import commons, ic
    from concept_amd.lib import ConceptGPUError
    from concept_amd.species import Component
    g = golden('lpt3_3lpt_dealias_g8')
    commons.load_params(str(g['param_text']))
    c = Component('matter', 'matter', N=512, mass=1.0)
    with pytest.raises(ConceptGPUError, match='3LPT is not implemented'):
        ic.realize_particles(c, 0.02, g['amplitudes'], g['amplitudes_θ'])


# ---- hand-over ---------------------------------------------------------------------------------------
def test_a_dealiased_3lpt_box_runs_through_a_time_loop_step():
    """from a P(k) table to Timeloop: a 16³ box with 3LPT and dealiasing (M = 24), PM gravity; the
    mesh force transfers no net momentum (|Σ Δmom| <= 1e-9 Σ|Δmom|, the bar of the 2LPT test)"""
    from concept_amd import commons, ic, stepper
    from concept_amd.species import Component
    g = 16
    p = commons.load_params({
        'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
        'output_times': {'a': (0.0202,)}, 'enable_Hubble': True,
        'potential_options': {'gridsize': {'gravity': {'pm': 2*g}}},
        'select_forces': {'all': {'gravity': 'pm'}},
        'realization_options': {'lpt': 3, 'backscale': True, 'dealias': True}})
    k = np.geomspace(1e-3, 10, 200)
    amplitudes = ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, g, L)
    D = 0.02
    growth = {'D1': D, 'f1': 1.0, 'D2': -3/7*D**2, 'f2': 2.0, 'D3a': -1/3*D**3, 'f3a': 3.0,
              'D3b': 10/21*D**3, 'f3b': 3.0, 'D3c': -1/7*D**3, 'f3c': 3.0}
    c = Component('matter', 'matter', N=g**3, mass=-1)
    ic.reset_tally()
    grids = ic.realize(c, p.a_begin, amplitudes, growth_factors=growth, extended=True)
    assert grids['gridsize_dealias'] == 24 and grids['Φ3'] is not None
    assert c.mass == pytest.approx(p.ρ_mbar*L**3/g**3, rel=1e-14)
    pos0, mom0 = c.host('pos'), c.host('mom')
    cell = L/g
    lattice = (np.stack(np.meshgrid(*[np.arange(g)]*3, indexing='ij'), -1).reshape(-1, 3) + .5)*cell
    d = np.abs(pos0 - lattice)
    assert 0.01*cell < np.minimum(d, L - d).max() < 2*cell and np.abs(mom0).max() > 0
    steps = []
    loop = stepper.Timeloop([c], on_step=lambda lp: steps.append(lp.cosmo.a))
    loop.run()
    assert len(steps) >= 1 and loop.cosmo.a == pytest.approx(0.0202, rel=1e-12)
    pos, mom = c.host('pos'), c.host('mom')
    assert c.N_local == g**3 and np.array_equal(np.sort(c.host('ids')), np.arange(g**3))
    assert (pos >= 0).all() and (pos < L).all() and np.isfinite(mom).all()
    kicks = mom - mom0
    assert np.abs(kicks).max() > 0
    assert np.abs(kicks.sum(0)).max() <= 1e-9*np.abs(kicks).sum(0).max()
