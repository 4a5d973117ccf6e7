"""Host logic of interactions.interpolate_upstream (no GPU): the one upstream interpolation of
gravity, power spectra and 2D renders (mesh.py:492-635 with add_upstream_to_global_slabs,
mesh.py:654-711).  get_mesh is replaced by a factory of recording stubs, one per (grid size,
role); the whole sequence of mesh calls is compared with literal lists, and every contribution
or factor with the expression written out here in the reference's order, bit for bit.

The lists are those the two former copies (the upstream half of particle_mesh_general and
analysis.interpolate_upstream) gave on the same stubs, with one exception: tile-sorted
components under the outputs' weight (`test_tile_sorted_first`) used to be zeroed and
deposited directly; they now take the tiled deposit as under gravity's."""
import types

import pytest

BOX = 613.7
A_SCALE = 0.37
MASS = {'A': 1.7, 'B': 0.43}
W_EFF = {'A': 0.11, 'B': -0.23, 'F': 0.31}
SDT = {'1': 0.0173, ('a**(-3*w_eff-1)', 'A'): 0.0291, ('a**(-3*w_eff-1)', 'B'): 0.0317,
       ('a**(-3*w_eff-1)', 'F'): 0.0269}
PARAMS = types.SimpleNamespace(boxsize=BOX, nghosts=2, cell_centered=True)
SC = (0, 0, 0)

# (weight, roles, device) as gravity, power spectra and renders pass them
CALLERS = {
    'gravity': ('a²ρ', ('global', 'upstream'), 'cuda:7'),
    'powerspec': ('ρ', ('powerspec', 'powerspec upstream'), None),
    'render2D': ('ρ', ('render2D', 'render2D upstream'), None),
}


class StubMesh:
    def __init__(self, log, gridsize, role, device, dist):
        self.log, self.gridsize, self.role, self.device = log, gridsize, role, device
        self.boxsize, self.nghosts = BOX, 2
        self.dist, self.nprocs, self.ghost_layers = dist, (2 if dist else 1), 3

    def _record(self, method, *arguments):
        self.log.append((self.role, self.gridsize, method, arguments))

    def zero(self):
        self._record('zero')

    def deposit(self, pos, contribution):
        self._record('deposit', pos, contribution)

    def deposit_tiled(self, pos, tile_offset, contribution, accumulate=False):
        self._record('deposit_tiled', pos, tile_offset, contribution, accumulate)

    def deposit_general(self, pos, contribution, order=2, shift=(0.0, 0.0, 0.0)):
        self._record('deposit_general', pos, contribution, order, shift)

    def fluid_add(self, fluid, factor=1.0, operation='+='):
        self._record('fluid_add', fluid, factor, operation)

    def fold_ghosts(self, general=False):
        self._record('fold_ghosts', general)

    def fft_forward(self):
        self._record('fft_forward')

    def nullify_nyquist(self):
        self._record('nullify_nyquist')

    def fourier_operate(self, deconv_order=0, nlattice=1, shift=(0.0, 0.0, 0.0), diff_dim=-1):
        self._record('fourier_operate', deconv_order, nlattice, shift)
        return self

    def copy_modes_from(self, source, deconv_order=0, nlattice=1, shift=(0.0, 0.0, 0.0),
                        operation='='):
        self._record('copy_modes_from', (source.role, source.gridsize), deconv_order, nlattice,
                     shift, operation)


class StubFactory:
    """stands in for get_mesh: one recording stub per (grid size, role)"""

    def __init__(self, dist=False):
        self.log, self.meshes, self.dist = [], {}, dist

    def __call__(self, gridsize, boxsize, nghosts=2, cell_centered=True, interp_order=2,
                 device=None, role='global'):
        assert (boxsize, nghosts, cell_centered, interp_order) == (BOX, 2, True, 2)
        key = (gridsize, role)
        if key not in self.meshes:
            self.meshes[key] = StubMesh(self.log, gridsize, role, device, self.dist)
        assert self.meshes[key].device == device
        return self.meshes[key]


def particles(name, own_gridsize=16, tile_sorted_on=None, device=None):
    """what interpolate_upstream reads of a particle component; tile_sorted_on: the grid size
    of the mesh its memory is in exact tile order of"""
    tile_mesh = None
    if tile_sorted_on is not None:
        tile_mesh = types.SimpleNamespace(gridsize=tile_sorted_on, boxsize=BOX, nghosts=2,
                                          device=device)
    return types.SimpleNamespace(
        name=name, representation='particles', mass=MASS[name], pos=f'{name}.pos',
        params=PARAMS, w_eff=lambda a: W_EFF[name], tiles_exact=tile_mesh is not None,
        tile_mesh=tile_mesh, tile_table=f'{name}.table' if tile_mesh is not None else None,
        _store=types.SimpleNamespace(mesh=types.SimpleNamespace(gridsize=own_gridsize)))


def fluid(name, gridsize):
    return types.SimpleNamespace(
        name=name, representation='fluid', mass=-1.0, gridsize=gridsize, ϱ=f'{name}.ϱ',
        params=PARAMS, w_eff=lambda a: W_EFF[name])


def weight_of(quantity):
    """the two weights as their callers write them"""
    if quantity == 'a²ρ':
        return lambda c: SDT['a**(-3*w_eff-1)', c.name]/SDT['1']
    a = A_SCALE
    return lambda c: a**(-3*(1 + c.w_eff(a=a)))


def contribution(quantity, name, gridsize):
    """interpolate_particles (mesh.py:1543-1573) in the reference's order"""
    if quantity == 'a²ρ':
        contribution = SDT['a**(-3*w_eff-1)', name]/SDT['1']
    else:
        contribution = A_SCALE**(-3*(1 + W_EFF[name]))
    contribution *= MASS[name]
    fft_factor = float(gridsize)**(-3)
    contribution_factor = fft_factor*(gridsize/BOX)**3
    contribution *= contribution_factor
    return contribution


def fluid_factor(quantity, name, gridsize):
    """add_fluid_to_grid (mesh.py:1712-1718) in the reference's order"""
    factor = float(gridsize)**(-3)
    if quantity == 'a²ρ':
        factor *= SDT['a**(-3*w_eff-1)', name]/SDT['1']
    else:
        factor *= A_SCALE**(-3*(1 + W_EFF[name]))
    return factor


def run(monkeypatch, caller, components, gridsizes_upstream, gridsize_global, order, interlace,
        deconvolve=True, dist=False):
    from concept_amd import interactions
    quantity, roles, device = CALLERS[caller]
    factory = StubFactory(dist)
    monkeypatch.setattr(interactions, 'get_mesh', factory)
    slab = interactions.interpolate_upstream(
        components, gridsizes_upstream, gridsize_global, weight_of(quantity), order, deconvolve,
        interlace, roles=roles, device=device)
    assert (slab.role, slab.gridsize) == (roles[0], gridsize_global)
    assert {role for _, role in factory.meshes} <= set(roles)
    return factory.log


@pytest.mark.parametrize('caller', CALLERS)
def test_two_components_cic(monkeypatch, caller):
    """(a) two particle components on the global grid, CIC, 'sc', not tile-sorted"""
    q, (G, U), dev = CALLERS[caller]
    log = run(monkeypatch, caller, [particles('A'), particles('B')], [16, 16], 16, 2, 'sc')
    assert log == [
        (G, 16, 'zero', ()),
        (G, 16, 'deposit', ('A.pos', contribution(q, 'A', 16))),
        (G, 16, 'deposit', ('B.pos', contribution(q, 'B', 16))),
        (G, 16, 'fold_ghosts', (False,)),
        (G, 16, 'fft_forward', ()),
        (G, 16, 'nullify_nyquist', ()),
        (G, 16, 'fourier_operate', (2, 1, SC)),
    ]


@pytest.mark.parametrize('caller', CALLERS)
def test_pcs_interlaced(monkeypatch, caller):
    """(b) PCS on 'bcc': a pass per sub-lattice, the second onto the mesh of the upstream role"""
    q, (G, U), dev = CALLERS[caller]
    log = run(monkeypatch, caller, [particles('A'), particles('B')], [16, 16], 16, 4, 'bcc')
    cA, cB = contribution(q, 'A', 16), contribution(q, 'B', 16)
    shifted = (-0.5, -0.5, -0.5)
    assert log == [
        (G, 16, 'zero', ()),
        (G, 16, 'deposit_general', ('A.pos', cA, 4, SC)),
        (G, 16, 'deposit_general', ('B.pos', cB, 4, SC)),
        (G, 16, 'fold_ghosts', (True,)),
        (G, 16, 'fft_forward', ()),
        (G, 16, 'nullify_nyquist', ()),
        (G, 16, 'fourier_operate', (4, 2, SC)),
        (U, 16, 'zero', ()),
        (U, 16, 'deposit_general', ('A.pos', cA, 4, shifted)),
        (U, 16, 'deposit_general', ('B.pos', cB, 4, shifted)),
        (U, 16, 'fold_ghosts', (True,)),
        (U, 16, 'fft_forward', ()),
        (U, 16, 'nullify_nyquist', ()),
        (G, 16, 'copy_modes_from', ((U, 16), 4, 2, shifted, '+=')),
    ]


@pytest.mark.parametrize('caller', CALLERS)
def test_two_grid_sizes(monkeypatch, caller):
    """(c) an upstream grid of twice the global size: the global size goes first, the larger
    grid arrives through copy_modes_from '+='; with nothing on the global grid, through '='
    into a fresh mesh of the global role"""
    q, (G, U), dev = CALLERS[caller]
    log = run(monkeypatch, caller, [particles('A'), particles('B')], [32, 16], 16, 2, 'sc',
              deconvolve=False)
    assert log == [
        (G, 16, 'zero', ()),
        (G, 16, 'deposit', ('B.pos', contribution(q, 'B', 16))),
        (G, 16, 'fold_ghosts', (False,)),
        (G, 16, 'fft_forward', ()),
        (G, 16, 'nullify_nyquist', ()),
        (G, 16, 'fourier_operate', (0, 1, SC)),
        (U, 32, 'zero', ()),
        (U, 32, 'deposit', ('A.pos', contribution(q, 'A', 32))),
        (U, 32, 'fold_ghosts', (False,)),
        (U, 32, 'fft_forward', ()),
        (U, 32, 'nullify_nyquist', ()),
        (G, 16, 'copy_modes_from', ((U, 32), 0, 1, SC, '+=')),
    ]
    log = run(monkeypatch, caller, [particles('A')], [32], 16, 2, 'sc')
    assert log == [
        (U, 32, 'zero', ()),
        (U, 32, 'deposit', ('A.pos', contribution(q, 'A', 32))),
        (U, 32, 'fold_ghosts', (False,)),
        (U, 32, 'fft_forward', ()),
        (U, 32, 'nullify_nyquist', ()),
        (G, 16, 'copy_modes_from', ((U, 32), 2, 1, SC, '=')),
    ]


@pytest.mark.parametrize('caller', CALLERS)
def test_fluid_then_particles(monkeypatch, caller):
    """(d) a fluid and a particle component of one grid size: the fluid first, onto the mesh
    of the global role; the particles' pass onto that of the upstream role"""
    q, (G, U), dev = CALLERS[caller]
    log = run(monkeypatch, caller, [particles('A'), fluid('F', 16)], [16, 16], 16, 2, 'sc')
    assert log == [
        (G, 16, 'fluid_add', ('F.ϱ', fluid_factor(q, 'F', 16), '=')),
        (G, 16, 'fft_forward', ()),
        (G, 16, 'nullify_nyquist', ()),
        (G, 16, 'fourier_operate', (0, 1, SC)),
        (U, 16, 'zero', ()),
        (U, 16, 'deposit', ('A.pos', contribution(q, 'A', 16))),
        (U, 16, 'fold_ghosts', (False,)),
        (U, 16, 'fft_forward', ()),
        (U, 16, 'nullify_nyquist', ()),
        (G, 16, 'copy_modes_from', ((U, 16), 2, 1, SC, '+=')),
    ]


@pytest.mark.parametrize('caller', CALLERS)
def test_tile_sorted_first(monkeypatch, caller):
    """(e) a tile-sorted and an unsorted component, CIC on 'sc': the tiled deposit goes first
    and assigns the mesh, nothing is zeroed.  (Under the outputs' weight the former copy gave
    zero, deposit A, deposit B: the one intended difference.)  Any other order or lattice
    takes the general deposit whatever the memory order."""
    q, (G, U), dev = CALLERS[caller]
    components = [particles('A'), particles('B', tile_sorted_on=16, device=dev)]
    log = run(monkeypatch, caller, components, [16, 16], 16, 2, 'sc')
    assert log == [
        (G, 16, 'deposit_tiled', ('B.pos', 'B.table', contribution(q, 'B', 16), False)),
        (G, 16, 'deposit', ('A.pos', contribution(q, 'A', 16))),
        (G, 16, 'fold_ghosts', (False,)),
        (G, 16, 'fft_forward', ()),
        (G, 16, 'nullify_nyquist', ()),
        (G, 16, 'fourier_operate', (2, 1, SC)),
    ]
    both = [particles('A', tile_sorted_on=16, device=dev),
            particles('B', tile_sorted_on=16, device=dev)]
    log = run(monkeypatch, caller, both, [16, 16], 16, 2, 'sc')
    assert log[:2] == [
        (G, 16, 'deposit_tiled', ('A.pos', 'A.table', contribution(q, 'A', 16), False)),
        (G, 16, 'deposit_tiled', ('B.pos', 'B.table', contribution(q, 'B', 16), True))]
    log = run(monkeypatch, caller, components, [16, 16], 16, 3, 'sc')
    assert log[:3] == [
        (G, 16, 'zero', ()),
        (G, 16, 'deposit_general', ('A.pos', contribution(q, 'A', 16), 3, SC)),
        (G, 16, 'deposit_general', ('B.pos', contribution(q, 'B', 16), 3, SC))]


@pytest.mark.parametrize('caller', CALLERS)
def test_unaligned_on_two_domains(monkeypatch, caller):
    """On two domains a component distributed by the slabs of another grid size is deposited
    directly onto a zeroed mesh — also where its memory is tile-sorted — and the fold is the
    general one."""
    q, (G, U), dev = CALLERS[caller]
    components = [particles('A', own_gridsize=16, tile_sorted_on=16, device=dev)]
    log = run(monkeypatch, caller, components, [32], 32, 2, 'sc', dist=True)
    assert log == [
        (G, 32, 'zero', ()),
        (G, 32, 'deposit', ('A.pos', contribution(q, 'A', 32))),
        (G, 32, 'fold_ghosts', (True,)),
        (G, 32, 'fft_forward', ()),
        (G, 32, 'nullify_nyquist', ()),
        (G, 32, 'fourier_operate', (2, 1, SC)),
    ]


@pytest.mark.parametrize('caller', CALLERS)
def test_refusals(monkeypatch, caller):
    """(f) a fluid of the wrong grid size, order 5, a reach beyond the halo on two domains"""
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError) as e:
        run(monkeypatch, caller, [particles('A'), fluid('F', 16)], [16, 32], 16, 2, 'sc')
    assert str(e.value) == ('add_fluid_to_grid() got component with global grid size 16 and '
                            'non-matching grid of global grid size 32')
    with pytest.raises(ConceptGPUError) as e:
        run(monkeypatch, caller, [particles('A')], [16], 16, 5, 'sc')
    assert str(e.value) == ('interpolate_particles() called with order = 5 '
                            '∉ {1 (NGP), 2 (CIC), 3 (TSC), 4 (PCS)}')
    with pytest.raises(ConceptGPUError) as e:
        run(monkeypatch, caller, [particles('A', own_gridsize=8)], [32], 32, 4, 'sc', dist=True)
    assert str(e.value) == (
        'A: its particles are distributed by the slabs of its 8^3 grid; on the 32^3 mesh they '
        'reach 4 layers beyond a slab face, the halo holds 3. Use grid sizes closer to each '
        'other or fewer domains.')


def test_gravity_general_path_calls_it(monkeypatch):
    """particle_mesh_general promotes the deconvolution, hands its suppliers to
    interpolate_upstream with the 'a²ρ' weight, the roles 'global' / 'upstream' and the
    receivers' device, and goes on at poisson_kernel"""
    from concept_amd import interactions

    class Reached(Exception):
        pass

    def poisson_kernel(self, *arguments):
        self._record('poisson_kernel', arguments[0])
        raise Reached
    monkeypatch.setattr(StubMesh, 'poisson_kernel', poisson_kernel, raising=False)
    factory = StubFactory()
    monkeypatch.setattr(interactions, 'get_mesh', factory)
    components = [particles('A'), particles('B')]
    for c in components:
        c.device = 'cuda:7'
        c.potential_gridsizes = {'gravity': {'pm': types.SimpleNamespace(upstream=16,
                                                                         downstream=16)}}
    PARAMS_G = types.SimpleNamespace(boxsize=BOX, nghosts=2, cell_centered=True, G_Newton=1.0)
    for c in components:
        c.params = PARAMS_G
    with pytest.raises(Reached):
        interactions.particle_mesh_general(
            components, components, 16, 'a²ρ', 'gravity', 'pm', 'gravity', 3, True, True, 'sc',
            'sc', SDT, ('a**(-3*w_eff)', 'component'))
    assert factory.log == [
        ('global', 16, 'zero', ()),
        ('global', 16, 'deposit_general', ('A.pos', contribution('a²ρ', 'A', 16), 3, SC)),
        ('global', 16, 'deposit_general', ('B.pos', contribution('a²ρ', 'B', 16), 3, SC)),
        ('global', 16, 'fold_ghosts', (True,)),
        ('global', 16, 'fft_forward', ()),
        ('global', 16, 'nullify_nyquist', ()),
        ('global', 16, 'fourier_operate', (0, 1, SC)),   # both deconvolutions promoted ...
        ('global', 16, 'poisson_kernel', (6,)),          # ... to the global one
    ]
