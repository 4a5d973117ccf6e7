"""The LPT realisation on the GPU (csrc/cg_lpt.hip, concept_amd/ic.py): each kernel against the
plain numpy references of tests/lpt_refs.py, the whole realisation against the reference's own
(tests/golden/lpt_*.npz), two closed-form second-order potentials, and the hand-over to the
time loop.

Bars.  A k-space kernel evaluates the reference's expression in the reference's order, so it may
differ from numpy only through cos / sin of the lattice phase (a few ulp): 1e-14 of the largest
value.  Particle displacement is x + f·ψ with both roundings kept: bit-identical.  Everything
that goes through the transforms: the project's 1e-12 (README) — of a cell for positions, of
max |mom| for momenta, of the Φ⁽¹⁾ scale for Φ⁽²⁾."""
import glob
import os

import numpy as np
import pytest

import lpt_refs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, 'lpt_*.npz')))
L = 100.0


def meshes(g, n, boxsize=L):
    from concept_amd.mesh import PotentialMesh
    return [PotentialMesh(g, boxsize) for _ in range(n)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, ref, bar):
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f'max error {err:.3e} = {err/scale:.3e} of the scale {scale:.3e} (bar {bar:.0e})')
    return err <= bar*scale


# ---- cg_lpt_potential -------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['1lpt_g8', '1lpt_g12', '2lpt_bcc2_g8', '2lpt_bcc2_g12',
                                  '1lpt_fixed_shift_g12'])
def test_potential_against_the_golden(golden, case):
    from concept_amd import commons, ic
    g = golden('lpt_' + case)
    p = commons.load_params(str(g['param_text']))
    n = int(g['gridsize'])
    shift = (0, 0, 0)
    if int(g['components_total']) == 2:
        shift = ic.lattice_shifts('bcc', p.cell_centered)[int(g['components_tally'])]
    noise, Φ1 = meshes(n, 2)
    noise.upload_fourier(g['noise'])
    nyq = n//2
    for key, table, factor in (('Phi1', 'amplitudes', -1), ('Phi1_theta', 'amplitudes_θ', 1)):
        Φ1.zero()
        Φ1.lpt_potential(noise, dev(g[table]), shift, factor)
        got = Φ1.fetch_fourier()
        assert close(got, g[key], 1e-14)
        assert close(got, lpt_refs.potential(g['noise'], g[table], shift, factor, L), 1e-14)
        # the origin and every Nyquist plane are exactly 0.0
        assert not got[0, 0, :2].any()
        assert not got[nyq].any() and not got[:, nyq].any() and not got[:, :, 2*nyq:].any()
        if p.primordial_amplitude_fixed:
            # |Φ|·k_f²·k2 = |amplitude| mode by mode
            ki, kj, kk = lpt_refs.wave_numbers(n)
            k2 = (ki**2 + kj**2 + kk**2)
            live = lpt_refs.alive(n)
            re, im = lpt_refs.split(got)
            lhs = np.hypot(re, im)*(2*np.pi/L)**2*k2
            rhs = np.abs(g[table])[np.minimum(k2, len(g[table]) - 1)]
            assert np.abs(lhs - rhs)[live].max() <= 1e-14*rhs.max()
    # in place without amplitudes: laplacian_inverse alone
    Φ1.upload_fourier(g['noise'])
    Φ1.lpt_potential(Φ1, None, factor=0.37)
    assert close(Φ1.fetch_fourier(), lpt_refs.potential(g['noise'], None, (0, 0, 0), 0.37, L),
                 1e-14)


def test_potential_refuses_a_wrong_table():
    from concept_amd.lib import ConceptGPUError
    a, b = meshes(8, 2)
    with pytest.raises(ConceptGPUError, match=r'27 amplitudes for grid size 8, which needs '
                                              r'3\*\(nyquist - 1\)\*\*2 \+ 1 = 28'):
        a.lpt_potential(b, dev(np.zeros(27)))
    c, = meshes(12, 1)
    with pytest.raises(ConceptGPUError, match='differ in grid size or domain'):
        a.lpt_potential(c, None)


# ---- cg_lpt_diff -------------------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', [12, 16])
def test_diff_first_and_second_derivatives(golden, gridsize):
    """negative frequencies and the Nyquist planes included: the source is dense random there"""
    rng = np.random.default_rng(gridsize)
    slab = rng.normal(size=(gridsize, gridsize, gridsize + 2))
    src, dst = meshes(gridsize, 2)
    src.upload_fourier(slab)
    nyq = gridsize//2
    cases = [(i, -1, 1.0) for i in range(3)] + [(i, j, 1.0) for i in range(3)
                                                for j in range(i, 3)]
    cases += [(1, -1, -2.5), (2, 0, 0.125)]
    for dim0, dim1, factor in cases:
        dst.upload_fourier(np.full_like(slab, 7.0))
        dst.lpt_diff(src, dim0, dim1, factor)
        got = dst.fetch_fourier()
        ref = lpt_refs.diff(slab, dim0, dim1, factor, L)
        assert np.array_equal(got, ref) or close(got, ref, 1e-15), (dim0, dim1, factor)
        assert not got[0, 0, :2].any()
        assert not got[nyq].any() and not got[:, nyq].any() and not got[:, :, 2*nyq:].any()
    assert np.array_equal(src.fetch_fourier(), slab)
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError, match=r'dimensions \(3, -1\) outside 0..2'):
        dst.lpt_diff(src, 3)


# ---- cg_lpt_product ------------------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', [12, 16])
def test_product_ops_factors_and_padding(gridsize):
    """the whole buffers are pre-filled with NaN: rows of padding and the unused row stay NaN,
    the payload never sees them"""
    import torch
    rng = np.random.default_rng(3)
    g = gridsize
    out, a, b = meshes(g, 3)
    fields = [rng.normal(size=(g, g, g)) for _ in range(3)]
    rows = out.layer_doubles//out.pad

    def fill(mesh, field):
        native = np.full((g, rows, out.pad), np.nan)
        native[:, :g, :g] = field
        mesh.layers_write(0, g, dev(native))
    for operation, factor in (('=', 1.0), ('+=', 1.0), ('-=', 1.0), ('=', -1.0), ('+=', 0.3),
                              ('-=', 1.7)):
        for m, f in zip((out, a, b), fields):
            fill(m, f)
        out.lpt_product(a, b, operation, factor)
        v = fields[1]*fields[2]
        if factor != 1:
            v = factor*v
        ref = {'=': v, '+=': fields[0] + v, '-=': fields[0] - v}[operation]
        got = out.fetch_real()
        assert np.array_equal(got[:, :, :g], ref), (operation, factor)
        buf = torch.empty(g*out.layer_doubles, dtype=torch.float64, device='cuda')
        out.layers_read(0, g, buf)
        native = buf.cpu().numpy().reshape(g, rows, out.pad)
        assert np.isnan(native[:, :g, g:]).all() and np.isnan(native[:, g:]).all()
    # a square: both factors one mesh, the output a third
    fill(a, fields[1])
    out.lpt_product(a, a, '=')
    assert np.array_equal(out.fetch_real()[:, :, :g], fields[1]*fields[1])


# ---- cg_lpt_displace -------------------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', [8, 12, 16, 40])
def test_displace_is_bit_identical(gridsize):
    import torch
    from concept_amd.lib import ConceptGPUError
    rng = np.random.default_rng(gridsize)
    g, n = gridsize, gridsize**3
    psi, = meshes(g, 1)
    rows = psi.layer_doubles//psi.pad
    native = np.full((g, rows, psi.pad), np.nan)
    native[:, :g, :g] = rng.normal(size=(g, g, g))
    psi.layers_write(0, g, dev(native))
    field = psi.fetch_real()[:, :, :g]
    assert np.array_equal(field, native[:, :g, :g])
    for index_bgn in (0, 5):
        pos0 = rng.uniform(0, L, (n + index_bgn + 3, 3))
        mom0 = rng.normal(size=pos0.shape)
        for dim, pf, mf in ((0, 1.0, 0.0), (1, 0.0, 0.731), (2, 1.0, -3.25e3), (1, 0.4, 1.0)):
            pos, mom = dev(pos0), dev(mom0)
            psi.lpt_displace(pos if pf else None, mom if mf else None, dim, pf, mf, index_bgn)
            pos_ref, mom_ref = lpt_refs.displace(field, pos0, mom0, index_bgn, dim, pf, mf)
            assert np.array_equal(pos.cpu().numpy(), pos_ref), (index_bgn, dim, pf, mf)
            assert np.array_equal(mom.cpu().numpy(), mom_ref), (index_bgn, dim, pf, mf)
    # n = 0 with NULL arrays
    from concept_amd import lib
    lib.check(lib.raw().cg_lpt_displace(psi._ctx, None, None, 0, 0, 0, 1.0, 1.0))
    with pytest.raises(ConceptGPUError, match=rf'7 particles for a lattice of {g}\*\*3 cells'):
        lib.check(lib.raw().cg_lpt_displace(psi._ctx, None, None, 7, 0, 0, 1.0, 1.0))
    with pytest.raises(ConceptGPUError, match='rows'):
        psi.lpt_displace(dev(np.zeros((n - 1, 3))), None, 0, 1.0, 0.0)


def test_wrap_and_lattice_expressions_on_the_device():
    """the torch expressions chosen over kernels give numpy's bits on the GPU too"""
    import torch
    from concept_amd import ic
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.uniform(-L, 2*L, 4000), [0.0, -0.0, L, -1e-20, -1e-300, 2*L, -L,
                                                     np.nextafter(L, 0), np.nextafter(L, 2*L)]])
    got = ic.wrap_positions(dev(x), L).cpu().numpy()
    ref = np.mod(x, L)
    ref[ref == L] = 0
    assert np.array_equal(got, ref) and np.all((got >= 0) & (got < L))
    for g in (12, 40):
        for c in (0.0, 0.5, -0.5):
            got = ((c + torch.arange(g, dtype=torch.float64, device='cuda'))*(L/g)).cpu().numpy()
            assert np.array_equal(got, (c + np.arange(g, dtype=np.float64))*(L/g))


# ---- end to end ----------------------------------------------------------------------------------------
def realize(g, p, mass=None):
    from concept_amd import ic
    from concept_amd.species import Component
    n = int(g['gridsize'])
    c = Component('matter', 'matter', N=n**3, mass=float(g['mass']) if mass is None else mass)
    ic.n_particles_realized.update(components_tally=int(g['components_tally']),
                                   components_total=int(g['components_total']),
                                   particles_tally=int(g['id_bgn']))
    growth = dict(zip(g['growth_keys'].tolist(), g['growth_values'].tolist()))
    grids = ic.realize_particles(c, float(g['a']), g['amplitudes'], g['amplitudes_θ'], growth)
    return c, grids


@pytest.mark.parametrize('case', CASES)
def test_realize_particles_against_the_golden(golden, case):
    from concept_amd import commons, ic
    g = golden('lpt_' + case)
    p = commons.load_params(str(g['param_text']))
    n = int(g['gridsize'])
    c, grids = realize(g, p)
    pos, mom, ids = c.host('pos'), c.host('mom'), c.host('ids')
    assert np.array_equal(ids, g['ids'])
    d = np.abs(pos - g['pos'])
    d = np.minimum(d, L - d).max()/(L/n)
    e = np.abs(mom - g['mom']).max()/np.abs(g['mom']).max()
    print(f'{case}: positions within {d:.3e} of a cell, momenta within {e:.3e} of max |mom|')
    assert d <= 1e-12 and e <= 1e-12
    assert (pos >= 0).all() and (pos < L).all()
    assert ic.n_particles_realized['particles_tally'] == int(g['id_bgn']) + n**3
    assert ic.n_particles_realized['components_tally'] == int(g['components_tally']) + 1
    # the potentials the reference had at the end, off the planes nothing reads
    live = np.repeat(lpt_refs.alive(n), 2, axis=2)
    assert close(grids['Φ1'].fetch_fourier()*live, g['Phi1'], 1e-14)
    if 'Phi2' in g.files:
        ref = g['Phi2']*live
        got = grids['Φ2'].fetch_fourier()*live
        err = np.abs(got - ref).max()/np.abs(g['Phi1']).max()
        print(f'Φ2 within {err:.3e} of the Φ1 scale')
        assert err <= 1e-12
    # a second run gives the same bits
    c2, _ = realize(g, p)
    assert np.array_equal(c2.host('pos'), pos) and np.array_equal(c2.host('mom'), mom)


def test_mass_left_unset_becomes_the_mean_density_mass(golden):
    from concept_amd import commons
    g = golden('lpt_1lpt_backscale_g8')
    p = commons.load_params(str(g['param_text']))
    c, _ = realize(g, p, mass=-1)
    assert c.mass == pytest.approx(float(g['mass']), rel=1e-14)
    assert np.abs(c.host('mom') - g['mom']).max() <= 1e-12*np.abs(g['mom']).max()


# ---- analytic, independent of the reference ---------------------------------------------------------
def phi2_of(noise_slab, g):
    """Φ⁽¹⁾ = ∇⁻²(noise) with unit amplitudes and Φ⁽²⁾ with D2/D1² = 1 through the kernels, in
    the order of the driver; returns both as real-space fields divided by the transforms' g³"""
    Φ1, Φ2, t0, t1 = meshes(g, 4)
    t0.upload_fourier(noise_slab)
    amp = dev(np.ones(3*(g//2 - 1)**2 + 1))
    Φ1.lpt_potential(t0, amp, factor=-1)
    terms = [('=', (0, 0), (1, 1), -1.0), ('-=', (1, 1), (2, 2), 1.0), ('-=', (2, 2), (0, 0), 1.0),
             ('+=', (0, 1), (0, 1), 1.0), ('+=', (1, 2), (1, 2), 1.0), ('+=', (0, 2), (0, 2), 1.0)]
    for operation, x, y, factor in terms:
        t0.lpt_diff(Φ1, *x)
        t0.poisson_backward()
        t1.lpt_diff(Φ1, *y)
        t1.poisson_backward()
        Φ2.lpt_product(t0, t1, operation, factor)
    Φ2.fft_forward()
    Φ2.lpt_potential(Φ2, None, factor=float(g)**-3)
    phi1 = lpt_refs.to_real(Φ1.fetch_fourier())
    live = np.repeat(lpt_refs.alive(g), 2, axis=2)
    return phi1, lpt_refs.to_real(Φ2.fetch_fourier()*live)


def mode_slab(g, modes):
    """a real field Σ 2·A·cos(k⃗·x⃗) as its Fourier slab: modes = [((ki, kj, kk), A)], kk > 0 or
    the conjugate partner written too"""
    slab = np.zeros((g, g, g + 2))
    for (ki, kj, kk), A in modes:
        slab[kj % g, ki % g, 2*kk] = A
        if kk == 0:
            slab[-kj % g, -ki % g, 0] = A
    return slab


@pytest.mark.parametrize('gridsize', [12, 16])
def test_a_single_plane_wave_has_no_second_order_potential(gridsize):
    phi1, phi2 = phi2_of(mode_slab(gridsize, [((2, 0, 0), 0.8)]), gridsize)
    assert np.abs(phi1).max() > 0
    assert np.abs(phi2).max() <= 1e-12*np.abs(phi1).max()


@pytest.mark.parametrize('gridsize', [12, 16])
def test_two_crossed_waves_give_the_closed_form(gridsize):
    """δ = 2A cos(k_x x) + 2B cos(k_y y) with unit amplitudes: ∇²Φ⁽¹⁾ = -δ gives
    Φ⁽¹⁾ = (2A/k_x²) cos(k_x x) + (2B/k_y²) cos(k_y y); the only product left is
    -Φ,₀₀Φ,₁₁ = -4AB cos(k_x x) cos(k_y y), and ∇²Φ⁽²⁾ = that (D2/D1² = 1) gives
    Φ⁽²⁾ = 4AB cos(k_x x) cos(k_y y)/(k_x² + k_y²)."""
    g = gridsize
    A, B, mx, my = 0.8, -0.3, 2, 3
    phi1, phi2 = phi2_of(mode_slab(g, [((mx, 0, 0), A), ((0, my, 0), B)]), g)
    k_f = 2*np.pi/L
    x = (np.arange(g)*(L/g))
    cx = np.cos(mx*k_f*x)[:, None, None]
    cy = np.cos(my*k_f*x)[None, :, None]
    ones = np.ones((1, 1, g))
    ref1 = (2*A/(mx*k_f)**2*cx + 2*B/(my*k_f)**2*cy)*ones
    assert np.abs(phi1 - ref1).max() <= 1e-12*np.abs(ref1).max()
    ref2 = 4*A*B*cx*cy/((mx*k_f)**2 + (my*k_f)**2)*ones
    assert np.abs(phi2 - ref2).max() <= 1e-12*np.abs(ref1).max()
    assert np.abs(ref2).max() > 1e-3*np.abs(ref1).max()


# ---- hand-over ---------------------------------------------------------------------------------------
def test_a_2lpt_box_runs_through_a_time_loop_step():
    """from a P(k) table to Timeloop: a 16³ 2LPT box, PM gravity, a few base steps; the mesh force
    transfers no net momentum (|Σ Δmom| <= 1e-9 Σ|Δmom|, the bar of the fused pass's own test)"""
    from concept_amd import commons, ic, stepper
    from concept_amd.species import Component
    g = 16
    p = commons.load_params({
        'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
        'output_times': {'a': (0.0202,)}, 'enable_Hubble': True,
        'potential_options': {'gridsize': {'gravity': {'pm': 2*g}}},
        'select_forces': {'all': {'gravity': 'pm'}},
        'realization_options': {'lpt': 2, 'backscale': True}})
    k = np.geomspace(1e-3, 10, 200)
    amplitudes = ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, g, L)
    c = Component('matter', 'matter', N=g**3, mass=-1)
    ic.reset_tally()
    ic.realize_particles(c, p.a_begin, amplitudes,
                         growth_factors={'D1': 0.02, 'f1': 1.0, 'D2': -3/7*0.02**2, 'f2': 2.0})
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
