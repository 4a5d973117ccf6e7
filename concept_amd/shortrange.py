"""concept_amd.shortrange — host side of the P3M short-range tile sweep.

Counterpart of component_component(..., pairing_level='tile')
(interactions.py:122-329) with gravity_pairwise_shortrange (gravity.py:263-354),
including the adaptive rungs (per-rung factors, active rungs, jumped indices:
cg_shortrange_sweep_rungs), and of pairing_level='domain' with gravity_pairwise /
gravity_pairwise_nonperiodic (direct summation with and without the Ewald
correction, component_component_pp below).  The pair loops run in
libconcept_gpu.so (cg_shortrange.hip, cg_pp.hip)."""
import contextlib
import math
import os

import numpy as np
import torch

from . import commons
from .lib import ConceptGPUError
from .mesh import PotentialMesh, get_mesh

_tables = {}
PAIR_KEY = 'a**(-3*w_eff₀-3*w_eff₁-1)'


def get_softened_r3inv(r2, ϵ, kernel='spline'):
    """interactions.py:1847-1914"""
    if kernel == 'none':
        r3 = r2*math.sqrt(r2)
        return 0 if r3 == 0 else 1/r3
    if kernel == 'plummer':
        r2_softened = r2 + ϵ**2
        return 1/(r2_softened*math.sqrt(r2_softened))
    if kernel != 'spline':
        raise ConceptGPUError(f'Softening kernel "{kernel}" not understood')
    h = 2.8*ϵ
    r = math.sqrt(r2)
    if r >= h:
        return 1/(r2*r)
    u = r/h
    if u < 0.5:
        return 32/h**3*(1./3. + u**2*(-6./5. + u))
    return 32/(3*r**3)*(u**3*(2 + u*(-9./2. + u*(18./5. - u))) - 3./480.)


def get_shortrange_table(softening, scale, range_, tablesize, kernel, device):
    """gravity.py:373-424.  Tabulated on the host (4096 entries), cached, kept in HBM."""
    key = (softening, scale, range_, tablesize, kernel, str(device))
    hit = _tables.get(key)
    if hit is not None:
        return hit
    maxr2 = (1 + 1/tablesize)*range_**2  # gravity.py:437
    r_tabulation = np.sqrt(np.linspace(0, maxr2, tablesize))
    table = np.empty(tablesize, dtype=np.float64)
    inv_scale = 1/scale
    for i in range(tablesize - 1):
        r2 = float(0.5*(r_tabulation[i]**2 + r_tabulation[i + 1]**2))
        r = math.sqrt(r2)
        x = r*inv_scale
        r3_inv = 1/(r2*r)
        table[i] = (
            - r3_inv*(1/math.sqrt(commons.π)*x*math.exp(-(0.5*x)**2) + (math.erfc(0.5*x) - 1))
            - get_softened_r3inv(r2, softening, kernel)
        )
    table[tablesize - 1] = np.nan  # never accessed (gravity.py:416-421)
    out = (torch.tensor(table, device=device), maxr2)
    _tables[key] = out
    return out


def combine_softening_lengths(ϵᵢ, ϵⱼ):
    """interactions.py:1820-1830"""
    return 0.5*(ϵᵢ + ϵⱼ)


def _pair_integrals(ᔑdt_rungs, rec, sup):
    """ᔑdt_rungs['a**(-3*w_eff₀-3*w_eff₁-1)', receiver, supplier] as a 1-D array: one entry
    per rung index (main.py:1203-1215 fills 3*N_rungs - 1 of them); a plain number — what
    get_time_step_integrals() gives for a single step — counts as rung 0."""
    k = (PAIR_KEY, rec.name, sup.name)
    if k not in ᔑdt_rungs:
        raise ConceptGPUError(
            f'ᔑdt_rungs lacks the integral {k!r} (both orders of a component pair are needed)')
    integrals = np.atleast_1d(np.asarray(ᔑdt_rungs[k], dtype=np.float64))
    if integrals.ndim != 1:
        raise ConceptGPUError(f'ᔑdt_rungs[{k!r}] must be a number or a 1-D array of rung integrals')
    if rec.use_rungs and integrals.size < 3*rec.N_rungs - 1:
        raise ConceptGPUError(
            f'ᔑdt_rungs[{k!r}] holds {integrals.size} integrals, {3*rec.N_rungs - 1} '
            f'(3*N_rungs - 1) are needed with rungs in use')
    return integrals


sparse_sweeps = 0   # sweeps taken without a cell list (a handful of active receivers)
# meshes that took a sweep bounded by the rung populations (without a cell list, or by active
# receiver) since their CG_ERR_ACTIVE_OVERFLOW was looked at
by_receiver_meshes = {}
_deferred_checks = 0


@contextlib.contextmanager
def deferred_active_checks():
    """The sweeps inside leave CG_ERR_ACTIVE_OVERFLOW (more receivers on active rungs than the
    rung populations said: some of them got no kick) to the caller, who looks at the meshes
    of by_receiver_meshes later (the rung loop: once per base step, RungStepper._check_sweeps,
    so that its sub-steps do not wait for the GPU).  Outside, component_component() looks
    itself before it returns."""
    global _deferred_checks
    _deferred_checks += 1
    try:
        yield
    finally:
        _deferred_checks -= 1


def global_tiling(boxsize, tilesize, range_=None):
    """(nt, tile_extent) of the global gravity tiling (species.py:3943-3950, :607-609), at
    least 4 tiles across; range_: tiles narrower than this force range are refused too."""
    nt = int((boxsize/1)/tilesize*(1 + commons.machine_ϵ))
    if nt < 4:
        raise ConceptGPUError(
            'The global gravity tiling needs to have at least 4 tiles across the box in every '
            'direction. Consider lowering shortrange_params["gravity"]["tilesize"].')
    if range_ is not None and tilesize < range_*(1 - 1e-12):
        raise ConceptGPUError('shortrange_params: tilesize must be at least the range')
    return nt, boxsize/nt


def sweep_form(rec, multi):
    """Which sweep kicks the receiver `rec`, and the bound on its active rows where the sweep
    takes one: 'plain' (no rungs, or every rung active: then the rung sweep over a plain list),
    'sparse' (a handful, one domain: no cell list), 'by_cell' (by active receiver) or 'blocks'
    (the jumped rungs copied into list order).  rungs_N counts the active rows without looking
    (over all domains: an upper bound of this domain's, which is all the sweeps ask for).  The
    list a receiver gets and the sweep over it both follow from this one answer."""
    if not rec.use_rungs or rec.lowest_active_rung <= 0:
        return 'plain', None
    n_active = int(sum(rec.rungs_N[rec.lowest_active_rung:]))
    if not multi and n_active <= PotentialMesh.SHORTRANGE_SPARSE_MAX:
        return 'sparse', None
    if n_active <= PotentialMesh.SHORTRANGE_BY_CELL_MAX*rec.N:
        return 'by_cell', n_active
    return 'blocks', None


class _PairSweeps:
    """The state of one component_component() call: the components' cell lists, the suppliers'
    lists where they differ (several domains) and the rows of the sweeps without a list."""

    def __init__(self, mesh, receivers, multi, nt, tile_extent, G_Newton, ᔑdt_rungs):
        self.mesh, self.receivers, self.multi = mesh, receivers, multi
        self.nt, self.tile_extent = nt, tile_extent
        self.G_Newton, self.ᔑdt_rungs = G_Newton, ᔑdt_rungs
        self.cells, self.supp_cells, self.sparse_rows = {}, {}, {}

    def cells_of(self, c):
        """the component's cell list (built when a sweep first asks for it: a sub-step that
        kicks a handful of particles needs none)"""
        if id(c) not in self.cells:
            # (the sub-step's first pass over the particles, if the time loop left it to this
            # list: run by the list's counting pass on the particles it bins)
            taken = c.take_begin(self.mesh)
            # a receiver's list of a sub-step has the active rows first in every cell; the
            # sweep in blocks wants the jumped rung indices in list order too
            rungs, in_blocks = None, False
            if c.use_rungs and c in self.receivers:
                rungs = (c.rung_indices, c.rung_indices_jumped, c.lowest_active_rung)
                in_blocks = sweep_form(c, self.multi)[0] == 'blocks'
            self.cells[id(c)] = self.mesh.shortrange_cells(c.pos, self.nt, self.tile_extent,
                                                           rungs, in_blocks)
            if taken:
                c.begin_queued()
            self.supp_cells.setdefault(id(c), self.cells[id(c)])
        return self.cells[id(c)]

    def sweep(self, rec, sup, table, scaling, r2_max):
        mesh = self.mesh
        # compute_factors (gravity.py:51-64): G*m_r*m_s*ᔑdt_rungs[...][k] per rung k
        integrals = _pair_integrals(self.ᔑdt_rungs, rec, sup)
        if not rec.use_rungs:
            rc = self.cells_of(rec)
            self.cells_of(sup)
            mesh.shortrange_sweep_cells(
                rc, rec.Δmom, self.supp_cells[id(sup)], self.nt, table, scaling, r2_max,
                self.G_Newton*rec.mass*sup.mass*float(integrals[0]))
            return
        factors = commons.upload(self.G_Newton*rec.mass*sup.mass*integrals, rec.device)
        form, n_active = sweep_form(rec, self.multi)
        if form == 'sparse':
            # the sub-steps for the highest rungs (main.py:1347-1624).  Which rows is found on
            # the GPU, not trusted to the populations: every row on an active rung is swept
            # (none claimed too: the kernels leave at once when no row is valid), and more
            # than the sweep can take raise CG_ERR_ACTIVE_OVERFLOW
            if id(rec) not in self.sparse_rows:
                self.sparse_rows[id(rec)] = commons.sparse_rows(
                    rec.rung_indices >= rec.lowest_active_rung, mesh.SHORTRANGE_SPARSE_MAX)
            global sparse_sweeps
            sparse_sweeps += 1
            rec.flush_begin()
            sup.flush_begin()
            by_receiver_meshes[id(mesh)] = mesh
            mesh.shortrange_sparse(rec.pos, self.sparse_rows[id(rec)], rec.Δmom, sup.pos,
                                   table, scaling, r2_max, 0.0,
                                   (factors, rec.rung_indices_jumped), overflow_slot=True)
            return
        self.cells_of(sup)
        rc = self.cells_of(rec)
        if form == 'by_cell':
            by_receiver_meshes[id(mesh)] = mesh
        mesh.shortrange_sweep_cells(
            rc, rec.Δmom, self.supp_cells[id(sup)], self.nt, table, scaling, r2_max, 0.0,
            (factors, rec.rung_indices, rec.rung_indices_jumped, rec.lowest_active_rung),
            n_active)


def component_component(force, receivers, suppliers, ᔑdt_rungs, gridsize):
    """Short-range gravity of every (receiver, supplier) component pair, accumulated
    into the components' Δmom buffers (the caller applies them, main.py:1253-1262)."""
    if force != 'gravity':
        raise ConceptGPUError(f'short-range force "{force}" is not built')
    p = receivers[0].params
    sr = commons.resolve_shortrange(p, gridsize)
    nt, tile_extent = global_tiling(p.boxsize, sr['tilesize'], sr['range'])
    mesh = get_mesh(gridsize, p.boxsize, p.nghosts, p.cell_centered, 2, receivers[0].device)
    involved = list({id(c): c for c in list(receivers) + list(suppliers)}.values())
    for c in involved:
        if c.representation != 'particles':
            raise ConceptGPUError(f'{c.name}: only particle components have short-range forces')
        # (asked of the store, not through the attribute: reading c.Δmom would run a sub-step
        # pass the time loop has left to this call's cell list)
        if 'Δmom' not in c._store.cols:
            c.Δmom = torch.zeros_like(c.mom)
    multi = mesh.dist and mesh.nprocs > 1
    sweeps = _PairSweeps(mesh, receivers, multi, nt, tile_extent, p.G_Newton, ᔑdt_rungs)
    if multi:
        # On several domains every supplier component is extended by the neighbour ranks'
        # particles within the force range of this rank's slab (sendrecv_component,
        # communication.py:847-1130); positions only (see ship_boundary_positions).
        from .distributed import check_shortrange_fits, with_boundary_positions
        # (components own their particles by the slabs of their own grids: the faces of two
        # components differ by less than half a cell of the coarser one)
        slack = max(c._store.mesh.boxsize/c._store.mesh.gridsize for c in involved)
        for c in involved:
            check_shortrange_fits(c._store.mesh, sr['range'] + slack)
        for c in involved:
            # every involved component can act as supplier: s of sweep(r, s), and r of the
            # reciprocal sweep(s, r) when s is also a receiver
            sweeps.cells_of(c)
            supp_pos = with_boundary_positions(
                c._store.mesh, c.pos, sr['range']*(1 + 1e-9) + slack + 1e-9*p.boxsize)
            sweeps.supp_cells[id(c)] = mesh.shortrange_cells(supp_pos, nt, tile_extent)
    done = set()
    for r in receivers:
        for s in suppliers:
            pair = frozenset((id(r), id(s)))
            if pair in done:
                continue
            done.add(pair)
            softening = combine_softening_lengths(r.softening_length, s.softening_length)
            table, maxr2 = get_shortrange_table(softening, sr['scale'], sr['range'],
                                                sr['tablesize'], p.softening_kernel, r.device)
            scaling = (sr['tablesize'] - 1)/maxr2  # gravity.py:288
            r2_max = sr['range']**2                # gravity.py:286
            sweeps.sweep(r, s, table, scaling, r2_max)
            if r is not s and s in receivers:
                # the reference kicks both partners of a pair (Δmom_s -= ..., gravity.py:341-349)
                sweeps.sweep(s, r, table, scaling, r2_max)
    # a sweep bounded by the populations met more active receivers than they said: an error,
    # not a kick silently lost (one wait for the GPU; the rung loop defers it)
    if not _deferred_checks and by_receiver_meshes.pop(id(mesh), None) is not None:
        mesh.check_errors()


_ewald_grids = {}


def get_ewald_grid(p, device):
    """ewald.get_ewald_grid() (ewald.py:200-224): the octant table of the Ewald correction,
    tabulated once per (ewald_gridsize, device) on the GPU and kept in HBM (the reference
    caches it on disk)."""
    key = (p.ewald_gridsize, str(device))
    grid = _ewald_grids.get(key)
    if grid is None:
        mesh = get_mesh(16, p.boxsize, p.nghosts, p.cell_centered, 2, device, role='pp')
        grid = _ewald_grids[key] = mesh.ewald_tabulate(p.ewald_gridsize)
    return grid


def component_component_pp(force, receivers, suppliers, ᔑdt_rungs, periodic):
    """component_component(..., pairing_level='domain') (interactions.py:122-329) with
    gravity_pairwise (periodic, Ewald-corrected) or gravity_pairwise_nonperiodic
    (gravity.py:121-206, 491-560): direct summation, accumulated into the components' Δmom
    buffers (the caller applies them, main.py:1253-1262)."""
    if force != 'gravity':
        raise ConceptGPUError(f'direct summation of force "{force}" is not built')
    p = receivers[0].params
    dev = receivers[0].device
    mesh = get_mesh(16, p.boxsize, p.nghosts, p.cell_centered, 2, dev, role='pp')
    ewald_grid = get_ewald_grid(p, dev) if periodic else None
    for c in {id(c): c for c in list(receivers) + list(suppliers)}.values():
        if c.representation != 'particles':
            raise ConceptGPUError(f'{c.name}: only particle components take part in direct '
                                  'summation')
        if c.Δmom is None:
            c.Δmom = torch.zeros_like(c.mom)
    key = 'a**(-3*w_eff₀-3*w_eff₁-1)'

    def all_positions(sup):
        """The supplier's particles of EVERY domain, this domain's first (the reference pairs
        every domain with every other, interactions.py:398-590; direct summation is O(N²)
        anyway, so the positions are simply gathered)."""
        comm = sup.comm
        if comm is None or comm.world == 1:
            return sup.pos
        counts = comm.all_gather_ints([sup.N_local])[:, 0].tolist()
        everything = comm.all_gather_rows(sup.pos.contiguous())
        start = int(sum(counts[:comm.rank]))
        return torch.cat([sup.pos, everything[:start], everything[start + sup.N_local:]])
    done = set()
    for r in receivers:
        for s in suppliers:
            pair = frozenset((id(r), id(s)))
            if pair in done:
                continue
            done.add(pair)
            softening = combine_softening_lengths(r.softening_length, s.softening_length)

            def kick(rec, sup, same):
                # compute_factors (gravity.py:51-64): G*m_r*m_s*ᔑdt_rungs[...][k] per rung k
                integrals = _pair_integrals(ᔑdt_rungs, rec, sup)
                rungs, factor = None, p.G_Newton*rec.mass*sup.mass*float(integrals[0])
                if rec.use_rungs:
                    factors = commons.upload(p.G_Newton*rec.mass*sup.mass*integrals, rec.device)
                    rungs = (factors, rec.rung_indices, rec.rung_indices_jumped,
                             rec.lowest_active_rung)
                    factor = 0.0
                mesh.pp_kick(rec.pos, rec.Δmom, all_positions(sup), same, ewald_grid, softening,
                             p.softening_kernel, factor, rungs)
            kick(r, s, r is s)
            if r is not s and s in receivers:
                kick(s, r, False)  # the reference kicks both partners of a pair
