"""Initial conditions: 1LPT / 2LPT / 3LPT particle realisation and the realisation of the fluid
variables ϱ and J (ic.py:67-232, 297-477, 599-627, 708-764, 928-2280 of the reference).

The reference gets two things from CLASS — a table of amplitudes T(k)·ζ(k) indexed by k² and a
handful of growth factors — and does everything after that on meshes.  Here both are inputs
(`amplitudes_from_power` makes the table from a tabulated P(k)) and the mesh work runs on the
GPU (csrc/cg_lpt.hip through PotentialMesh.lpt_*):

    noise (host, numpy's own generators: the reference's random streams, number for number;
           or with noise_on='device' the same streams drawn on the GPU, csrc/cg_noise.hip)
      -> Φ⁽¹⁾ = ∇⁻²(amplitude·noise)            lpt_potential
      -> Ψ⁽¹⁾ᵢ = ∂ᵢΦ⁽¹⁾, back to real space      lpt_diff + the mesh's inverse transform
      -> positions += Ψ, momenta += factor·Ψ    lpt_displace
    2LPT: the six products of second derivatives of Φ⁽¹⁾ (lpt_diff, lpt_product) summed into
    the source of Φ⁽²⁾, transformed, ∇⁻², and displaced the same way.
    3LPT (extended=True): Φ⁽³ᵃ⁾, Φ⁽³ᵇ⁾ and the three A⁽³ᶜ⁾ᵢ from tables of terms (LptTerms), the
    last displaced by its curl.  Dealiasing (extended=True): every derivative is enlarged to
    M = 3N/2 (lpt_diff_enlarge), every product made there, nullified beyond the cube |k| < N/2
    (lpt_dealias_cube) and the last one shrunk into the potential (lpt_shrink_accumulate).

    fluids (realize_fluid, realize): the same noise
      -> amplitude·noise (ϱ) or amplitude·(-i kⁱ/k²)·noise (Jⁱ)   realize_grid
      -> back to real space                                       the mesh's inverse transform
      -> ϱ = ϱ_bar(1 + δ) or Jⁱ = a**(1 - 3w_eff)ϱ_bar(1 + w)uⁱ    fluid_from_mesh

    the shear of closure 'class' (realize_shear; the time loop's path is fluid.shear_sources):
      ϱ of the component itself, transformed forward                fluid_structure
      -> amplitude·(½δₘₙ - (3/2)kₘkₙ/k²)·ℱ[ϱ]                        realize_grid_tensor
      -> back to real space, ςₘₙ = ϱ_bar(1 + w)σₘₙ                  fluid_from_mesh
    the table is the caller's (amplitudes_from_transfer_ratio), as for the particles.

Out of scope, refused by name.  Particles: 3LPT and Orszag dealiasing unless extended=True,
non-Gaussianity, non-primordial structure, N without a cubic lattice.  Fluids: δP, ς from the
primordial noise or above boltzmann_order = 1; realize_fluid and realize refuse ς and closure
'class' as they always did: ς is opted into through realize_shear.  Both: several domains."""
import contextlib
import math

import numpy as np
import torch

from . import comm as _comm
from . import commons
from .commons import is_selected, π
from .lib import ConceptGPUError


# ---- pseudo-random numbers (ic.py:67-232) ------------------------------------------------
class PseudoRandomNumberGenerator:
    """The reference's generator: a numpy bit generator seeded with the salted seed, children
    by spawn key, every distribution drawn through a cache of `cache_size` numbers.  draws()
    hands out the next n numbers of a distribution at once — the same numbers, in the same
    order, as n single draws."""
    streams = {name: attr for name, attr in vars(np.random).items()
               if isinstance(attr, type) and issubclass(attr, np.random.BitGenerator)
               and attr is not np.random.BitGenerator}

    def __init__(self, seed=None, stream=None, cache_size=2**12, salt=True):
        if stream is None:
            stream = commons.params.random_generator if commons.params else 'PCG64DXSM'
        if salt and isinstance(seed, int):
            seed += int(π*1e+8)  # no seeds of many zero bits
            seed += 137          # the reference's hand-picked offset
        if not isinstance(seed, np.random.SeedSequence):
            seed = np.random.SeedSequence(seed)
        self.seed = seed
        self.stream = stream
        self.cache_size = cache_size
        bit_generator = self.streams.get(stream)
        if bit_generator is None:
            names = ', '.join(f'"{s}"' for s in self.streams)
            raise ConceptGPUError(f'Pseudo-random bit generator "{stream}" not available in '
                                  f'NumPy. The available ones are {names}.')
        self.generator = np.random.Generator(bit_generator(self.seed))
        self._cache = {}  # distribution -> (numbers, how many of them are used)

    def spawn(self, spawn_key=0):
        spawn_key = tuple(spawn_key) if isinstance(spawn_key, (tuple, list)) else (spawn_key,)
        seed = np.random.SeedSequence(self.seed.entropy,
                                      spawn_key=(self.seed.spawn_key + spawn_key))
        return type(self)(seed, self.stream, self.cache_size)

    def draws(self, distribution, n):
        """the next n unit-scale numbers of 'uniform' [0, 1), 'gaussian' or 'rayleigh'"""
        out = np.empty(n, dtype=np.float64)
        cache, used = self._cache.get(distribution, (None, self.cache_size))
        filled = 0
        while filled < n:
            if used == self.cache_size:
                cache = {'uniform': lambda: self.generator.uniform(0, 1, size=self.cache_size),
                         'gaussian': lambda: self.generator.normal(0, 1, size=self.cache_size),
                         'rayleigh': lambda: self.generator.rayleigh(1, size=self.cache_size),
                         }[distribution]()
                used = 0
            take = min(n - filled, self.cache_size - used)
            out[filled:filled + take] = cache[used:used + take]
            filled += take
            used += take
        self._cache[distribution] = (cache, used)
        return out

    def uniform(self, low=0, high=1, n=1):
        return low + self.draws('uniform', n)*(high - low)

    def gaussian(self, scale=1, n=1):
        return self.draws('gaussian', n)*scale

    def rayleigh(self, scale=1, n=1):
        return self.draws('rayleigh', n)*scale


# ---- the Fourier space-filling curve (mesh.py:3053-3096) -----------------------------------
def fourier_curve_key(ki, kj, kk):
    """The place of mode (ki, kj, kk) on the curve that fills Fourier space outwards from the
    origin, shell by shell of max(|ki|, |kj|, kk) (get_fourier_curve_key); int64 arrays."""
    ki, kj, kk = (np.asarray(v, dtype=np.int64) for v in (ki, kj, kk))
    ki_abs, kj_abs = np.abs(ki), np.abs(kj)
    kl = np.where(ki_abs > kj_abs, ki, np.where(ki_abs < kj_abs, kj, np.maximum(ki, kj)))
    kl_abs = np.abs(kl)
    s = np.where(kl_abs < kk, kk, kl_abs + (kl > 0))
    return np.select(
        [kk == s, kj == -s, ki == -s, ki != s - 1],
        [kj + s*(2*ki + s*(4*s + 2) + 1),
         kk + s*(ki + s*(4*s - 1)),
         kk + s*(kj + s*(4*s - 3)),
         kk + s*(ki + s*(4*s - 5) + 2)],
        kk + s*(kj + s*(4*s - 7) + 3))


def _curve_order_slice(gridsize):
    """(ki, kk) of one j-slice off the Nyquist planes in visiting order: the curve's order for
    the slice kj = 0, whatever the slice (fourier_curve_slice_loop, mesh.py:2984-3044)"""
    nyquist = gridsize//2
    ki, kk = np.meshgrid(np.arange(-nyquist + 1, nyquist), np.arange(nyquist), indexing='ij')
    ki, kk = ki.ravel(), kk.ravel()
    order = np.argsort(fourier_curve_key(ki, np.zeros_like(ki), kk), kind='stable')
    return ki[order], kk[order]


def _curve_order(gridsize):
    """(ki, kj, kk) of the whole grid off the Nyquist planes in the curve's order
    (fourier_curve_loop, mesh.py:2909-2962)"""
    nyquist = gridsize//2
    full = np.arange(-nyquist + 1, nyquist)
    ki, kj, kk = (v.ravel() for v in np.meshgrid(full, full, np.arange(nyquist), indexing='ij'))
    order = np.argsort(fourier_curve_key(ki, kj, kk), kind='stable')
    return ki[order], kj[order], kk[order]


# ---- primordial noise (ic.py:928-1163) ---------------------------------------------------------
def generate_primordial_noise(gridsize, fixed_amplitude=False, phase_shift=0, params=None):
    """The Fourier slab of primordial white noise of one domain, double[j][i][gridsize + 2] in
    the reference's transposed layout: r·exp(iθ) with r Rayleigh(1/√2) (1 when fixed_amplitude)
    and θ uniform in [-π, π) (+ phase_shift), imprinted by params.primordial_noise_imprinting
    ('distributed': streams per j-slice spawned by kj; 'simple': one stream pair along the
    whole curve), the kk = 0 plane Hermitian, the origin zero; the Nyquist planes stay zero."""
    p = params or commons.params
    if p is None:
        raise ConceptGPUError('no parameters loaded: call concept_amd.commons.load_params()')
    g = int(gridsize)
    if g < 2 or g % 2:
        raise ConceptGPUError(f'generate_primordial_noise(): grid size {g} must be even and ≥ 2')
    nyquist = g//2
    slab = np.zeros((g, g, g + 2), dtype=np.float64)
    prng_amplitudes_common = PseudoRandomNumberGenerator(
        p.random_seeds['primordial amplitudes'], p.random_generator)
    prng_phases_common = PseudoRandomNumberGenerator(
        p.random_seeds['primordial phases'], p.random_generator)
    scale = 1/math.sqrt(2)

    def polar(prng_r, prng_θ, n):
        r = 1.0 if fixed_amplitude else prng_r.rayleigh(scale, n)
        return r, prng_θ.uniform(-π, π, n)

    def finalize(r, θ, mask):
        θ = θ[mask]
        if phase_shift:
            θ = θ + phase_shift
        r = r if fixed_amplitude else r[mask]
        return r*np.cos(θ), r*np.sin(θ)

    scheme = p.primordial_noise_imprinting
    if scheme == 'simple':
        ki, kj, kk = _curve_order(g)
        r, θ = polar(prng_amplitudes_common, prng_phases_common, ki.size)
        lower_x_zdc = (ki < 0) | ((ki == 0) & (kj < 0))
        imprint = (kk != 0) | lower_x_zdc
        imprint_conj = (kk == 0) & lower_x_zdc
        re, im = finalize(r, θ, imprint)
        slab[kj[imprint] % g, ki[imprint] % g, 2*kk[imprint]] = re
        slab[kj[imprint] % g, ki[imprint] % g, 2*kk[imprint] + 1] = im
        re, im = finalize(r, θ, imprint_conj)
        slab[-kj[imprint_conj] % g, -ki[imprint_conj] % g, 0] = +re
        slab[-kj[imprint_conj] % g, -ki[imprint_conj] % g, 1] = -im
    elif scheme == 'distributed':
        spawn_key_offset = 2**32  # negative seeds not allowed
        ki, kk = _curve_order_slice(g)
        i = ki % g
        i_conj = -ki % g
        for j in range(g):
            kj = j - (g if j >= nyquist else 0)
            if kj == -nyquist:
                continue
            r, θ = polar(prng_amplitudes_common.spawn(spawn_key_offset + kj),
                         prng_phases_common.spawn(spawn_key_offset + kj), ki.size)
            r_conj, θ_conj = polar(prng_amplitudes_common.spawn(spawn_key_offset - kj),
                                   prng_phases_common.spawn(spawn_key_offset - kj), ki.size)
            # off the kk = 0 plane every point takes its own numbers; on it the lower x half
            # (ki < 0, or ki = 0 and kj < 0) does, and the other half takes the conjugate of
            # what the slice at -kj drew for the reflected point
            on_zdc = (kk == 0)
            imprint = ~on_zdc | (ki < 0) | ((ki == 0) & (kj < 0))
            imprint_conj = on_zdc & ~((ki > 0) | ((ki == 0) & (-kj > 0)))
            re, im = finalize(r, θ, imprint)
            slab[j, i[imprint], 2*kk[imprint]] = re
            slab[j, i[imprint], 2*kk[imprint] + 1] = im
            re, im = finalize(r_conj, θ_conj, imprint_conj)
            slab[j, i_conj[imprint_conj], 0] = +re
            slab[j, i_conj[imprint_conj], 1] = -im
    else:
        raise ConceptGPUError(f'primordial_noise_imprinting = "{scheme}" not implemented')
    slab[0, 0, 0] = slab[0, 0, 1] = 0  # nullify_modes(slab, 'origin')
    return slab


# ---- primordial noise on the device (csrc/cg_noise.hip) ------------------------------------------
PCG_CHEAP_MULTIPLIER = 0xda942042e4dd58b5  # PCG64DXSM: state' = a·state + inc mod 2¹²⁸
_MASK64, _MASK128 = 2**64 - 1, 2**128 - 1
_noise_tables = {}  # (device, 'jump' | gridsize) -> device tensor


def _words128(*values):
    """128-bit integers as pairs of 64-bit words, low word first"""
    return [w for v in values for w in (v & _MASK64, v >> 64)]


def pcg64dxsm_jump_table(n):
    """uint64[n + 1][4]: row k holds (aᵏ, Sₖ = 1 + a + … + aᵏ⁻¹) mod 2¹²⁸, low words first.
    k steps of PCG64DXSM take `state` to aᵏ·state + Sₖ·inc, whatever the stream and the seed."""
    rows, power, series = [], 1, 0
    for _ in range(n + 1):
        rows.append(_words128(power, series))
        series = (series*PCG_CHEAP_MULTIPLIER + 1) & _MASK128
        power = (power*PCG_CHEAP_MULTIPLIER) & _MASK128
    return np.array(rows, dtype=np.uint64)


def noise_order_table(gridsize):
    """int32[(g - 1)·g/2][2]: the point (ki, kk) the t-th draw of a j-slice belongs to"""
    ki, kk = _curve_order_slice(gridsize)
    return np.ascontiguousarray(np.stack([ki, kk], axis=1).astype(np.int32))


def noise_stream_table(gridsize, fixed_amplitude=False, params=None):
    """uint64[g - 1][8]: for every spawn key κ = -nyquist + 1 … nyquist - 1 of the 'distributed'
    scheme the 128-bit state and increment of the amplitude stream and of the phase stream
    (low words first), as numpy seeds them.  Every stream appears once: the slice kj = κ draws
    it for itself and the slice kj = -κ as its conjugate stream.  With fixed amplitudes the
    amplitude streams are not made (polar() does not draw them either): their words are 0."""
    p = params or commons.params
    if p is None:
        raise ConceptGPUError('no parameters loaded: call concept_amd.commons.load_params()')
    _check_noise_device_scope(p)
    nyquist = int(gridsize)//2
    spawn_key_offset = 2**32
    commons_ = [None if fixed_amplitude else PseudoRandomNumberGenerator(
                    p.random_seeds['primordial amplitudes'], p.random_generator),
                PseudoRandomNumberGenerator(p.random_seeds['primordial phases'],
                                            p.random_generator)]
    table = np.zeros((2*nyquist - 1, 8), dtype=np.uint64)
    for row, κ in enumerate(range(-nyquist + 1, nyquist)):
        for n, common in enumerate(commons_):
            if common is None:
                continue
            state = common.spawn(spawn_key_offset + κ).generator.bit_generator.state['state']
            table[row, 4*n:4*n + 4] = _words128(state['state'], state['inc'])
    return table


def _check_noise_device_scope(p):
    scheme = p.primordial_noise_imprinting
    if scheme == 'simple':
        raise ConceptGPUError(
            'primordial noise on the device: primordial_noise_imprinting = "simple" is not '
            'implemented (its two streams run along the whole curve; "distributed" is)')
    if scheme != 'distributed':
        raise ConceptGPUError(f'primordial_noise_imprinting = "{scheme}" not implemented')
    if p.random_generator != 'PCG64DXSM':
        raise ConceptGPUError(
            f'primordial noise on the device: random_generator = "{p.random_generator}" is not '
            'implemented (the bit generator "PCG64DXSM" is)')


def _check_noise_on(component, noise_on):
    """what noise_on='device' needs beyond the scope of the realisation itself"""
    if noise_on == 'host':
        return
    if noise_on != 'device':
        raise ConceptGPUError(f"{component.name}: noise_on = {noise_on!r} is neither 'host' nor "
                              "'device'")
    if _comm.active() is not None or getattr(component, 'nprocs', 1) > 1:
        raise ConceptGPUError(
            f"{component.name}: noise_on='device' with an active comm process group: the "
            'primordial noise of several domains is not generated on the device')
    _check_noise_device_scope(component.params)


def _noise_table_dev(device, key, make):
    table = _noise_tables.get((device, key))
    if table is None:
        array = make()
        if array.dtype == np.uint64:
            array = array.view(np.int64)
        table = _noise_tables[device, key] = torch.from_numpy(array).to(device)
    return table


def generate_primordial_noise_device(mesh, fixed_amplitude=False, phase_shift=0, params=None):
    """The slab generate_primordial_noise(mesh.gridsize, ...) returns, as upload_fourier would
    leave it in the Fourier view of `mesh`, drawn on the device from the same random streams
    (csrc/cg_noise.hip): the same modes, zeros on the Nyquist planes and at the origin, the
    kk = 0 plane Hermitian.  The amplitudes and the uniform numbers are numpy's to the bit; cos,
    sin and the ziggurat's rare log1p and exp are the device library's.  The 'distributed'
    scheme on PCG64DXSM (the defaults) and one domain; anything else is refused.  Returns the
    mesh."""
    from .lib import raw
    p = params or commons.params
    if p is None:
        raise ConceptGPUError('no parameters loaded: call concept_amd.commons.load_params()')
    g = int(mesh.gridsize)
    if g < 2 or g % 2:
        raise ConceptGPUError(f'generate_primordial_noise_device(): grid size {g} must be even '
                              'and ≥ 2')
    if mesh.dist or _comm.active() is not None:
        raise ConceptGPUError('generate_primordial_noise_device() with an active comm process '
                              'group: the primordial noise of several domains is not generated '
                              'on the device')
    streams = noise_stream_table(g, fixed_amplitude, p)
    trip = int(raw().cg_noise_trip())
    jump = _noise_table_dev(mesh.device, 'jump', lambda: pcg64dxsm_jump_table(trip))
    order = _noise_table_dev(mesh.device, g, lambda: noise_order_table(g))
    streams = torch.from_numpy(streams.view(np.int64)).to(mesh.device)
    return mesh.noise_generate(streams, order, jump, fixed_amplitude, phase_shift)


# ---- amplitudes (ic.py:599-627) ------------------------------------------------------------------
def amplitudes_from_power(k, P, gridsize, boxsize):
    """The k²-indexed table get_amplitudes hands to realize_grid, from a tabulated power
    spectrum: amplitudes[k2] = sqrt(P(k_f·√k2))·boxsize**(-1.5) for k2 = 1 .. 3(nyquist-1)²,
    P interpolated linearly in (log k, log P); amplitudes[0] = 0."""
    k, P = np.asarray(k, dtype=np.float64), np.asarray(P, dtype=np.float64)
    if k.ndim != 1 or k.shape != P.shape or k.size < 2 or np.any(np.diff(k) <= 0):
        raise ConceptGPUError('amplitudes_from_power(): k must be increasing, P of its length')
    nyquist = int(gridsize)//2
    k2_max = 3*(nyquist - 1)**2
    k_fundamental = 2*π/boxsize
    amplitudes = np.zeros(k2_max + 1, dtype=np.float64)
    k_magnitude = k_fundamental*np.sqrt(np.arange(1, k2_max + 1, dtype=np.float64))
    if k2_max and (k_magnitude[0] < k[0] or k_magnitude[-1] > k[-1]):
        raise ConceptGPUError(
            f'amplitudes_from_power(): the table covers k in [{k[0]}, {k[-1]}], the grid needs '
            f'[{k_magnitude[0]}, {k_magnitude[-1]}]')
    amplitudes[1:] = np.sqrt(np.exp(np.interp(np.log(k_magnitude), np.log(k), np.log(P)))
                             )*boxsize**(-1.5)
    return amplitudes


# ---- lattices (mesh.py:78-182) ----------------------------------------------------------------
def lattice_shifts(kind, cell_centered=True):
    """The shifts, in grid units and as applied to particles, of the primitive simple cubic
    lattices of a 'sc', 'bcc' or 'fcc' lattice: -½ on cell-centred grids, +½ on cell-vertex."""
    s = (1 - 2*bool(cell_centered))*0.5
    return {'sc': [(0, 0, 0)],
            'bcc': [(0, 0, 0), (s, s, s)],
            'fcc': [(0, 0, 0), (0, s, s), (s, 0, s), (s, s, 0)]}[kind]


def preic_lattice(N):
    """'sc', 'bcc', 'fcc' for N, N/2, N/4 cubic, else '' (species.py:1107-1117)"""
    def iscubic(n):
        return round(n**(1/3))**3 == n
    if iscubic(N):
        return 'sc'
    if N % 2 == 0 and iscubic(N//2):
        return 'bcc'
    if N % 4 == 0 and iscubic(N//4):
        return 'fcc'
    return ''


# Record updated by realize_particles(), as in the reference (ic.py:1406-1411)
n_particles_realized = {'components_tally': 0, 'components_total': 0, 'particles_tally': 0}


def reset_tally():
    n_particles_realized.update(components_tally=0, components_total=0, particles_tally=0)


# ---- pre-initialisation (ic.py:2138-2223) ---------------------------------------------------------
def preinitialize_particles(component, n_particles=-1, index_bgn=0, id_bgn=0,
                            shift=(0, 0, 0)):
    """Rows [index_bgn, index_bgn + n_particles) of the component at the points of a simple
    cubic lattice (cell centres on cell-centred grids) moved by `shift` grid units, row
    (i·g + j)·g + k at point (i, j, k) with identifier id_bgn + that number, momenta zero.
    Torch expressions: (c + i)·(boxsize/g) in FP64 is the reference's value to the bit."""
    if component.representation != 'particles':
        return 0
    p = component.params
    if n_particles == -1:
        n_particles = component.N
    g = round(n_particles**(1/3))
    if g**3 != n_particles:
        raise ConceptGPUError(f'preinitialize_particles() called with non-cubic number of '
                              f'particles {n_particles}')
    if component.N_local < index_bgn + n_particles:
        raise ConceptGPUError('Component passed to preinitialize_particles() is too small')
    rows = slice(index_bgn, index_bgn + n_particles)
    pos = component.pos[rows].view(g, g, g, 3)
    index = torch.arange(g, dtype=torch.float64, device=pos.device)
    spacing = p.boxsize/g
    for dim, view in enumerate(((g, 1, 1), (1, g, 1), (1, 1, g))):
        c = (0 + 0.5*bool(p.cell_centered)) + shift[dim]
        pos[..., dim] = ((c + index)*spacing).view(view)
    component.ids[rows] = id_bgn + torch.arange(n_particles, dtype=torch.int64,
                                                 device=pos.device)
    component.mom[rows] = 0
    return n_particles


def wrap_positions(pos, boxsize):
    """pos = mod(pos, boxsize) with the reference's mod (commons.py:5108-5113): the remainder
    with the sign of boxsize, and 0 where that rounds to boxsize.  A torch expression."""
    pos.remainder_(boxsize)
    pos.masked_fill_(pos == boxsize, 0.0)
    return pos


# ---- the driver (ic.py:1199-1589) ---------------------------------------------------------------
GROWTH_FACTOR_KEYS = ('D1', 'f1', 'D2', 'f2', 'D3a', 'f3a', 'D3b', 'f3b', 'D3c', 'f3c')


def realization_options(component):
    p = component.params
    return {key: is_selected(component, d) for key, d in p.realization_options.items()}


def _check_scope(component, options, extended=False):
    name = component.name
    lpt = options['lpt']
    if extended:
        if lpt not in {1, 2, 3}:
            raise ConceptGPUError(f'{name}: realize_particles() called with attempted {lpt}LPT, '
                                  'though only 1LPT, 2LPT and 3LPT are implemented')
    else:
        if lpt == 3:
            raise ConceptGPUError(f'{name}: realization_options["lpt"] = 3: 3LPT is not '
                                  'implemented (1LPT and 2LPT are)')
        if lpt not in {1, 2}:
            raise ConceptGPUError(f'{name}: realize_particles() called with attempted {lpt}LPT, '
                                  'though only 1LPT and 2LPT are implemented')
        if options['dealias']:
            raise ConceptGPUError(f'{name}: realization_options["dealias"]: Orszag dealiasing of '
                                  'the LPT products is not implemented')
    if options['nongaussianity'] != 0:
        raise ConceptGPUError(f'{name}: realization_options["nongaussianity"] = '
                              f'{options["nongaussianity"]}: non-Gaussian initial conditions are '
                              'not implemented')
    if options['structure'] != 'primordial':
        raise ConceptGPUError(f'{name}: Can only realize particles using the primordial '
                              f'structure, not "{options["structure"]}"')
    if component.representation != 'particles':
        raise ConceptGPUError(f'{name}: realize_particles() called with a non-particle '
                              'component (fluid realisation is not implemented)')
    if not preic_lattice(component.N):
        raise ConceptGPUError(
            f'Cannot initialize particle component {name} with N = {component.N} on a lattice, '
            'as neither of {N, N/2, N/4} is a cubic number')
    if _comm.active() is not None or getattr(component, 'nprocs', 1) > 1:
        raise ConceptGPUError(f'{name}: realize_particles() with an active comm process group: '
                              'multi-GPU realisation is not implemented')


class _Stopwatch:
    """event pairs around the passes of one realisation, summed by kind (tools/ic_time.py)"""
    def __init__(self, timings):
        self.timings, self.pairs = timings, []

    @contextlib.contextmanager
    def __call__(self, kind):
        if self.timings is None:
            yield
            return
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        yield
        e1.record()
        self.pairs.append((kind, e0, e1))

    def finish(self):
        if self.timings is None:
            return
        torch.cuda.synchronize()
        for kind, e0, e1 in self.pairs:
            self.timings[kind] = self.timings.get(kind, 0.0) + e0.elapsed_time(e1)
            self.timings[kind + ' passes'] = self.timings.get(kind + ' passes', 0) + 1


# ---- the potentials above the first (ic.py:1539-2103) ---------------------------------------------
def dealias_gridsize(gridsize):
    """the size of the enlarged grids of Orszag's 3/2 rule, made even (ic.py:1322-1323)"""
    gridsize_dealias = (gridsize*3)//2
    return gridsize_dealias + (gridsize_dealias & 1)


def _term(output, operation, factor, *potentials):
    """(output, operation, factor, ((potential, dim0, dim1), ...)): one term of the source of
    an LPT potential, the dimensions of a derivative sorted as handle_lpt_term sorts them"""
    return (output, operation, float(factor),
            tuple((name,) + tuple(sorted(dims)) for name, *dims in potentials))


# ∇²Φ⁽²⁾ = D⁽²⁾/(D⁽¹⁾)² (-Φ,₀₀Φ,₁₁ - Φ,₁₁Φ,₂₂ - Φ,₂₂Φ,₀₀ + Φ,₀₁² + Φ,₁₂² + Φ,₂₀²), Φ = Φ⁽¹⁾
# (ic.py:1554-1575)
LPT_TERMS_2 = (
    _term('Φ2', '=', -1, ('Φ1', 0, 0), ('Φ1', 1, 1)),
    _term('Φ2', '-=', 1, ('Φ1', 1, 1), ('Φ1', 2, 2)),
    _term('Φ2', '-=', 1, ('Φ1', 2, 2), ('Φ1', 0, 0)),
    _term('Φ2', '+=', 1, ('Φ1', 0, 1), ('Φ1', 0, 1)),
    _term('Φ2', '+=', 1, ('Φ1', 1, 2), ('Φ1', 1, 2)),
    _term('Φ2', '+=', 1, ('Φ1', 2, 0), ('Φ1', 2, 0)),
)
# ∇²Φ⁽³ᵃ⁾ = D⁽³ᵃ⁾/(D⁽¹⁾)³ (Φ,₂₀²Φ,₁₁ - Φ,₁₁Φ,₂₂Φ,₀₀ + Φ,₀₀Φ,₁₂² - 2Φ,₁₂Φ,₂₀Φ,₀₁ + Φ,₀₁²Φ,₂₂)
# (ic.py:1633-1652)
LPT_TERMS_3A = (
    _term('Φ3', '=', 1, ('Φ1', 2, 0), ('Φ1', 2, 0), ('Φ1', 1, 1)),
    _term('Φ3', '-=', 1, ('Φ1', 1, 1), ('Φ1', 2, 2), ('Φ1', 0, 0)),
    _term('Φ3', '+=', 1, ('Φ1', 0, 0), ('Φ1', 1, 2), ('Φ1', 1, 2)),
    _term('Φ3', '-=', 2, ('Φ1', 1, 2), ('Φ1', 2, 0), ('Φ1', 0, 1)),
    _term('Φ3', '+=', 1, ('Φ1', 0, 1), ('Φ1', 0, 1), ('Φ1', 2, 2)),
)
# ∇²Φ⁽³ᵇ⁾ = D⁽³ᵇ⁾/(D⁽¹⁾D⁽²⁾) (-½Φ⁽¹⁾,₂₂Φ⁽²⁾,₀₀ - ½Φ⁽²⁾,₀₀Φ⁽¹⁾,₁₁ - ½Φ⁽¹⁾,₁₁Φ⁽²⁾,₂₂ - ½Φ⁽²⁾,₂₂Φ⁽¹⁾,₀₀
#   - ½Φ⁽¹⁾,₀₀Φ⁽²⁾,₁₁ - ½Φ⁽²⁾,₁₁Φ⁽¹⁾,₂₂ + Φ⁽²⁾,₂₀Φ⁽¹⁾,₂₀ + Φ⁽²⁾,₀₁Φ⁽¹⁾,₀₁ + Φ⁽²⁾,₁₂Φ⁽¹⁾,₁₂)  (ic.py:1711-1739)
LPT_TERMS_3B = (
    _term('Φ3', '=', -0.5, ('Φ1', 2, 2), ('Φ2', 0, 0)),
    _term('Φ3', '-=', 0.5, ('Φ2', 0, 0), ('Φ1', 1, 1)),
    _term('Φ3', '-=', 0.5, ('Φ1', 1, 1), ('Φ2', 2, 2)),
    _term('Φ3', '-=', 0.5, ('Φ2', 2, 2), ('Φ1', 0, 0)),
    _term('Φ3', '-=', 0.5, ('Φ1', 0, 0), ('Φ2', 1, 1)),
    _term('Φ3', '-=', 0.5, ('Φ2', 1, 1), ('Φ1', 2, 2)),
    _term('Φ3', '+=', 1, ('Φ2', 2, 0), ('Φ1', 2, 0)),
    _term('Φ3', '+=', 1, ('Φ2', 0, 1), ('Φ1', 0, 1)),
    _term('Φ3', '+=', 1, ('Φ2', 1, 2), ('Φ1', 1, 2)),
)


def lpt_terms_3c(i):
    """∇²Aᵢ⁽³ᶜ⁾ = D⁽³ᶜ⁾/(D⁽¹⁾D⁽²⁾) (Φ⁽²⁾,ⱼⱼΦ⁽¹⁾,ⱼₖ - Φ⁽¹⁾,ⱼₖΦ⁽²⁾,ₖₖ - Φ⁽¹⁾,ᵢⱼΦ⁽²⁾,ᵢₖ - Φ⁽¹⁾,ⱼⱼΦ⁽²⁾,ⱼₖ
    + Φ⁽²⁾,ⱼₖΦ⁽¹⁾,ₖₖ + Φ⁽²⁾,ᵢⱼΦ⁽¹⁾,ᵢₖ) with (i, j, k) cyclic (ic.py:1801-1830)"""
    j, k = (i + 1) % 3, (i + 2) % 3
    return (
        _term('Φ3', '=', 1, ('Φ2', j, j), ('Φ1', j, k)),
        _term('Φ3', '-=', 1, ('Φ1', j, k), ('Φ2', k, k)),
        _term('Φ3', '-=', 1, ('Φ1', i, j), ('Φ2', i, k)),
        _term('Φ3', '-=', 1, ('Φ1', j, j), ('Φ2', j, k)),
        _term('Φ3', '+=', 1, ('Φ2', j, k), ('Φ1', k, k)),
        _term('Φ3', '+=', 1, ('Φ2', i, j), ('Φ1', i, k)),
    )


def _gradient():
    """Ψᵢ = ∂ᵢΦ: (dimension of the derivative, its factor, dimension displaced)"""
    return tuple((i, 1.0, i) for i in range(3))


def _curl(i):
    """the part of Ψ⁽³ᶜ⁾ⱼ = ±∂ₖAᵢ that Aᵢ carries, with the sign of ic.py:1840-1847"""
    passes = []
    for j in range(3):
        if j == i:
            continue
        k = 3 - i - j
        passes.append((k, float(2*(k == (j + 1) % 3) - 1), j))
    return tuple(passes)


def lpt_orders(lpt):
    """What follows 1LPT, potential by potential in the reference's order (carryout_2lpt,
    carryout_3lpt_a, _b and three times _c): (name, terms, growth factor D, the potentials whose
    D⁽ⁿ⁾ divide it, growth rate f, displacement passes)."""
    orders = []
    if lpt >= 2:
        orders.append(('Φ2', LPT_TERMS_2, 'D2', lambda g: g['D1']**2, 'f2', _gradient()))
    if lpt >= 3:
        orders.append(('Φ3a', LPT_TERMS_3A, 'D3a', lambda g: g['D1']**3, 'f3a', _gradient()))
        orders.append(('Φ3b', LPT_TERMS_3B, 'D3b', lambda g: g['D1']*g['D2'], 'f3b',
                       _gradient()))
        for i in range(3):
            orders.append((f'A3c{i}', lpt_terms_3c(i), 'D3c', lambda g: g['D1']*g['D2'], 'f3c',
                           _curl(i)))
    return orders


class LptTerms:
    """handle_lpt_term (ic.py:1895-2057) driven by data, with the reference's book-keeping of
    what the temporary grids hold (`notes`), so that a derivative the next term needs is not made
    again.  One object per lattice; begin() at the start of every potential, as the reference
    makes its dict of grids anew there.

    potentials: name -> mesh in Fourier space.  tmps: the two temporary meshes of the
    realisation size; tmps_dealias: the two of the dealiasing size, or None.  A mesh is anything
    with the lpt_* and transform methods of PotentialMesh: the host tests pass recorders.

    Where the reference copies a derivative into the second temporary grid to square it
    (ic.py:2005-2009), the two names swap their grids instead and the product reads one grid
    twice: the names hold what the reference's hold, and no copy is made."""

    def __init__(self, potentials, tmps, tmps_dealias=None, watch=None):
        self.potentials = potentials
        self.dealias = tmps_dealias is not None
        self.grids = {f'tmp{n}': (tmp, tmps_dealias[n] if self.dealias else tmp)
                      for n, tmp in enumerate(tmps)}
        self.gridsize = tmps[0].gridsize
        self.gridsize_dealias = self.grids['tmp0'][1].gridsize
        self.fft_factor = float(self.gridsize_dealias)**(-3)
        self.watch = watch or _Stopwatch(None)
        self.notes = {}
        self.begin()

    def begin(self):
        self.order = sorted(self.grids)

    def take_tmp(self):
        """get_tmpgrid (ic.py:2063-2074): the first temporary grid, which then goes last"""
        name = self.order.pop(0)
        self.order.append(name)
        return name

    def release_tmp(self):
        """the realisation-size grid the displacement uses after a potential is built
        (ic.py:1583-1584): whatever it held is gone"""
        name = self.take_tmp()
        self.notes.pop(name, None)
        return self.grids[name][0]

    def diff_ifft(self, pot, name):
        """diff_ifft (ic.py:2093-2103) of a potential's derivative into the named grid"""
        Φ, (dim0, dim1) = self.potentials[pot[0]], (pot[1:] + (-1,))[:2]
        work = self.grids[name][1]
        with self.watch('k-space'):
            if self.dealias:
                work.lpt_diff_enlarge(Φ, dim0, dim1)
            else:
                work.lpt_diff(Φ, dim0, dim1)
        with self.watch('transforms'):
            work.poisson_backward()

    def __call__(self, term):
        output, operation, factor, pots = term
        n_pot = len(pots)
        if self.dealias:  # every dealiasing step but the last brings its own M⁻³ (ic.py:1956-1958)
            factor *= self.fft_factor**(n_pot - 2)
        notes = self.notes
        # reuse what the temporary grids hold (ic.py:1962-1984): the first potential in front
        # (it becomes the base grid), else the second at the back (the temporary grid)
        unique = list(dict.fromkeys(pots))
        for n, pot in enumerate(unique[:2]):
            if pot not in notes.values():
                continue
            name_reuse = next(name for name in notes if notes[name] == pot)
            others = [name for name in self.order if name != name_reuse]
            self.order = [name_reuse] + others if n == 0 else others + [name_reuse]
            break
        base = self.take_tmp()
        if notes.get(base) != pots[0]:
            self.diff_ifft(pots[0], base)
        notes.pop(base, None)
        tmp = self.take_tmp()
        Φ_out = self.potentials[output]
        for n, pot in enumerate(pots[1:], 1):
            factors = (base, tmp)
            if n == 1 and pot == pots[0]:
                self.grids[base], self.grids[tmp] = self.grids[tmp], self.grids[base]
                factors = (tmp, tmp)
            elif notes.get(tmp) != pot:
                self.diff_ifft(pot, tmp)
            notes[tmp] = pot
            x, y = (self.grids[name][1] for name in factors)
            work = self.grids[base][1]
            last = (n == n_pot - 1)
            with self.watch('products'):
                if last and not self.dealias:
                    # the last product and the move to the output grid (ic.py:2020-2057)
                    Φ_out.lpt_product(x, y, operation, factor)
                else:
                    work.lpt_product(x, y, '=')
            if self.dealias:
                with self.watch('transforms'):
                    work.fft_forward()
                if not last:  # ic.py:2023-2026
                    with self.watch('k-space'):
                        work.lpt_dealias_cube(self.gridsize)
                    with self.watch('transforms'):
                        work.poisson_backward()
        if self.dealias:  # shrink, staying in Fourier space, and move (ic.py:2029-2057)
            with self.watch('k-space'):
                Φ_out.lpt_shrink_accumulate(self.grids[base][1], operation, factor)


def carryout_lpt(orders, terms, growth_factors, a, H, mass, particles=(None, None, 0),
                 on_potential=None):
    """The potentials above the first for one lattice and their displacements (carryout_2lpt
    ... carryout_3lpt_c, ic.py:1539-1848).  orders: lpt_orders(lpt); terms: an LptTerms, which
    holds the meshes; particles: (pos, mom, index_bgn) for lpt_displace."""
    pos, mom, index_bgn = particles
    watch = terms.watch
    for name, term_list, D, denominator, f, passes in orders:
        Φ = terms.potentials[term_list[0][0]]
        potential_factor = terms.fft_factor*growth_factors[D]/denominator(growth_factors)
        velocity_factor = a*H*growth_factors[f]
        terms.begin()
        for term in term_list:
            terms(term)
        if not terms.dealias:
            with watch('transforms'):
                Φ.fft_forward()
        with watch('k-space'):
            Φ.lpt_potential(Φ, None, factor=potential_factor)
        if on_potential is not None:
            on_potential(name, Φ, potential_factor)
        tmp = terms.release_tmp()
        for dim_diff, factor, dim in passes:
            with watch('k-space'):
                tmp.lpt_diff(Φ, dim_diff, -1, factor)
            with watch('transforms'):
                tmp.poisson_backward()
            with watch('particles'):
                tmp.lpt_displace(pos, mom, dim, 1.0, velocity_factor*(a*mass), index_bgn)


def realize_particles(component, a, amplitudes, amplitudes_θ=None, growth_factors=None,
                      cosmology=None, components_all=None, timings=None, extended=False,
                      on_potential=None, noise_on='host'):
    """Realise a particle component at scale factor a (realize_particles, ic.py:1199-1400):
    particles on their lattice, displaced and boosted by 1LPT and, with
    realization_options['lpt'] = 2, 2LPT; positions wrapped into [0, boxsize).

    extended: carry out realization_options['lpt'] = 3 and ['dealias'] = True (Orszag's 3/2 rule
      on every product of grids) as well.  Without it both are refused by name, as they have
      been since the realisation was built and as the tests of that scope pin word for word; the
      wider scope is opted into, as the fluid solvers are.  ic.realize forwards the keyword.
    on_potential: called as on_potential(name, mesh, factor) after every potential above the
      first is built ('Φ2', 'Φ3a', 'Φ3b', 'A3c0', 'A3c1', 'A3c2': the last five share a mesh).

    amplitudes: the k²-indexed table of δ (amplitudes_from_power, or the caller's own transfer
      functions, signed as they wish); amplitudes_θ: that of θ, needed without back-scaling.
    growth_factors: dict with the reference's keys ('D1', 'f1', 'D2', 'f2', ...) at a; needed
      with back-scaling or 2LPT ('D3a', 'f3a', 'D3b', 'f3b', 'D3c', 'f3c' too with 3LPT).
    cosmology: an integration.Cosmology (H(a)); default: one of the component's parameters.
    components_all: every component of the run; those that are particles with mass -1 are the
      ones to be realised and decide the lattice of each (1: sc, 2: bcc, 4: fcc by tally).
    timings: a dict that receives milliseconds by kind of pass (synchronises).
    noise_on: 'host' draws the primordial noise with numpy and uploads the slab ('noise (host)'
      and 'upload' in timings); 'device' draws the same streams on the GPU into the mesh
      (generate_primordial_noise_device; 'noise (device)' in timings) — the 'distributed'
      scheme on PCG64DXSM and one domain, anything else is refused."""
    _check_noise_on(component, noise_on)
    options = realization_options(component)
    _check_scope(component, options, extended)
    p = component.params
    backscale, lpt = bool(options['backscale']), int(options['lpt'])
    dealias = bool(options['dealias']) and lpt >= 2  # 1LPT has no product to dealias
    if not backscale and amplitudes_θ is None:
        raise ConceptGPUError(f'{component.name}: without back-scaling the momenta come from '
                              'the amplitudes of θ: pass amplitudes_θ')
    growth_factors = dict(growth_factors or {})
    if backscale or lpt > 1:
        need = ('D1', 'f1') + (('D2', 'f2') if lpt > 1 else ()) + (
            ('D3a', 'f3a', 'D3b', 'f3b', 'D3c', 'f3c') if lpt > 2 else ())
        missing = [key for key in need if key not in growth_factors]
        if missing:
            raise ConceptGPUError(f'{component.name}: growth factors {missing} are needed')
    for key in GROWTH_FACTOR_KEYS:
        growth_factors.setdefault(key, math.nan)
    if cosmology is None:
        from .integration import Cosmology
        cosmology = Cosmology(p)
    # the lattice (ic.py:1231-1281)
    tally = n_particles_realized
    if tally['components_tally'] == 0:
        others = [c for c in (components_all or [component])
                  if c.representation == 'particles' and c.mass == -1]
        tally['components_total'] = len(others)
    kind = preic_lattice(component.N)
    shifts = lattice_shifts(kind, p.cell_centered)
    if kind == 'sc':
        kind_all = {2: 'bcc', 4: 'fcc'}.get(tally['components_total'])
        if kind_all is not None:
            shifts = lattice_shifts(kind_all, p.cell_centered)
            shifts = [shifts[tally['components_tally'] % len(shifts)]]
    n_particles = component.N//len(lattice_shifts(kind))
    gridsize = round(n_particles**(1/3))
    if gridsize % 2:
        raise ConceptGPUError(f'{component.name}: a lattice of {gridsize}³ particles: the '
                              'realisation grid must be even')
    if component.mass == -1:
        component.mass = component.ϱ_bar*p.boxsize**3/component.N
    amplitudes_dev = {0: _amplitudes_dev(component, amplitudes, gridsize)}
    if not backscale:
        amplitudes_dev[1] = _amplitudes_dev(component, amplitudes_θ, gridsize)
    watch = _Stopwatch(timings)
    # Φ⁽¹⁾ and one temporary grid; 2LPT: Φ⁽²⁾ and a second temporary grid; 3LPT: Φ⁽³⁾, which
    # holds Φ⁽³ᵃ⁾, Φ⁽³ᵇ⁾ and the three A⁽³ᶜ⁾ᵢ in turn; dealiasing: two enlarged temporary grids
    # (ic.py:1304-1325)
    from .mesh import get_mesh
    def grid(role, size=gridsize):
        return get_mesh(size, p.boxsize, p.nghosts, p.cell_centered, role=role,
                        device=component.device)
    Φ1, tmp0 = grid('lpt Φ1'), grid('lpt tmp0')
    Φ2, tmp1 = (grid('lpt Φ2'), grid('lpt tmp1')) if lpt >= 2 else (None, tmp0)
    Φ3 = grid('lpt Φ3') if lpt >= 3 else None
    potentials = {'Φ1': Φ1, 'Φ2': Φ2, 'Φ3': Φ3}
    gridsize_dealias = dealias_gridsize(gridsize) if dealias else gridsize
    tmps_dealias = None
    if dealias:
        tmps_dealias = (grid('lpt tmp0 dealias', gridsize_dealias),
                        grid('lpt tmp1 dealias', gridsize_dealias))
    noise = None
    if noise_on == 'host':
        with _host_timer(timings, 'noise (host)'):
            noise = generate_primordial_noise(gridsize, p.primordial_amplitude_fixed,
                                              p.primordial_phase_shift, p)
    mass = a**(-3*component.w_eff(a=a))*component.mass  # ic.py:2267
    H = cosmology.hubble(a)
    pos, mom = component.pos, component.mom
    index_bgn, id_bgn = 0, tally['particles_tally']

    def displace(Φ, tmp, pos_factor, mom_factor):
        """Ψᵢ = ∂ᵢΦ to real space (diff_ifft, ic.py:2093-2103), then displace_particles twice"""
        for dim in range(3):
            with watch('k-space'):
                tmp.lpt_diff(Φ, dim)
            with watch('transforms'):
                tmp.poisson_backward()
            with watch('particles'):
                tmp.lpt_displace(pos if pos_factor else None, mom if mom_factor else None, dim,
                                 pos_factor, mom_factor, index_bgn)

    for shift in shifts:
        with watch('particles'):
            preinitialize_particles(component, n_particles, index_bgn, id_bgn, shift)
        # 1LPT (carryout_1lpt, ic.py:1447-1509): ∇²Φ⁽¹⁾ = -δ; first θ, then δ
        velocity_factor = a*H*growth_factors['f1']
        uploaded = False
        for variable in range(1 - backscale, -1, -1):
            if not uploaded or tmp1 is tmp0:
                if noise is None:
                    with watch('noise (device)'):
                        generate_primordial_noise_device(tmp0, p.primordial_amplitude_fixed,
                                                         p.primordial_phase_shift, p)
                else:
                    with watch('upload'):
                        tmp0.upload_fourier(noise)
                uploaded = True
            with watch('k-space'):
                Φ1.lpt_potential(tmp0, amplitudes_dev[variable], shift, factor=2*variable - 1)
            if backscale:
                displace(Φ1, tmp1, 1.0, velocity_factor*(a*mass))
            elif variable == 0:
                displace(Φ1, tmp1, 1.0, 0.0)
            else:
                displace(Φ1, tmp1, 0.0, 1*(a*mass))
        if lpt >= 2:
            # 2LPT and 3LPT (ic.py:1352-1380): the notes start empty on every lattice
            terms = LptTerms(potentials, (tmp0, tmp1), tmps_dealias, watch)
            carryout_lpt(lpt_orders(lpt), terms, growth_factors, a, H, mass,
                         (pos, mom, index_bgn), on_potential)
        id_bgn += n_particles
        index_bgn += n_particles
    tally['particles_tally'] = id_bgn
    tally['components_tally'] += 1
    if id_bgn != component.N:
        component.use_ids = True  # not the running row numbers of this component
    with watch('particles'):
        wrap_positions(pos, p.boxsize)  # ic.py:1396-1398
    # the rows are new particles to everything that keeps state about them
    component.tile_mesh = None
    component.tiles_exact = False
    component._store.touch_mom()
    watch.finish()
    return {'Φ1': Φ1, 'Φ2': Φ2, 'Φ3': Φ3, 'gridsize': gridsize,
            'gridsize_dealias': gridsize_dealias}


# ---- fluids (ic.py:297-511, 708-764) ---------------------------------------------------------------
def _check_fluid_scope(component, variable, multi_index):
    name = component.name
    if component.representation != 'fluid':
        raise ConceptGPUError(f'realize_fluid() called with non-fluid component {name}')
    if variable not in (0, 1):
        raise ConceptGPUError(f'{name}: realize_fluid() got non-implemented variable = {variable} '
                              '(ϱ and J are implemented; ς, δP and the "class" closure are not)')
    if variable > component.boltzmann_order:
        raise ConceptGPUError(f'{name}: fluid variable {variable} exceeds the Boltzmann order '
                              f'{component.boltzmann_order} of the component (realisation from '
                              'the "class" closure is not implemented)')
    if variable == 1 and multi_index not in (0, 1, 2):
        raise ConceptGPUError(f'{name}: realize_fluid() of J needs multi_index 0, 1 or 2, not '
                              f'{multi_index!r}')
    if _comm.active() is not None or getattr(component, 'nprocs', 1) > 1:
        raise ConceptGPUError(f'{name}: realize_fluid() with an active comm process group: '
                              'multi-GPU realisation is not implemented')


def _realization_mesh(component, role):
    from .mesh import get_mesh
    p = component.params
    return get_mesh(component.gridsize, p.boxsize, p.nghosts, p.cell_centered, role=role,
                    device=component.device)


def realize_fluid(component, a, amplitudes, variable=0, multi_index=0, noise=None, timings=None,
                  noise_on='host'):
    """Realise one fluid scalar of a fluid component at scale factor a (realize_fluid,
    ic.py:400-477): ϱ (variable 0) or J[multi_index] (variable 1) from the primordial noise.

    amplitudes: the k²-indexed table (amplitudes_from_power) of δ for ϱ, of θ for J.
    noise: a mesh that holds the primordial noise in Fourier space (what an earlier call
      returned); without it the noise is generated on the host and uploaded, or with
      noise_on='device' on the GPU (as in realize_particles).
    timings: a dict that receives milliseconds by kind of pass (synchronises).
    Returns the noise mesh.  realization_options['structure'] plays no part: a variable within
    the Boltzmann order is realised from the primordial structure (ic.py:819-823)."""
    _check_noise_on(component, noise_on)
    _check_fluid_scope(component, variable, multi_index)
    p = component.params
    gridsize = component.gridsize
    amplitudes_dev = _amplitudes_dev(component, amplitudes, gridsize, 'a fluid grid of {}³ cells')
    watch = _Stopwatch(timings)
    if noise is None:
        noise = _realization_mesh(component, 'realize noise')
        if noise_on == 'device':
            with watch('noise (device)'):
                generate_primordial_noise_device(noise, p.primordial_amplitude_fixed,
                                                 p.primordial_phase_shift, p)
        else:
            with _host_timer(timings, 'noise (host)'):
                slab = generate_primordial_noise(gridsize, p.primordial_amplitude_fixed,
                                                 p.primordial_phase_shift, p)
            with watch('upload'):
                noise.upload_fourier(slab)
    elif noise.gridsize != gridsize:
        raise ConceptGPUError(f'{component.name}: a noise mesh of grid size {noise.gridsize} for '
                              f'a fluid of grid size {gridsize}')
    work = _realization_mesh(component, 'realize work')
    with watch('k-space'):
        work.realize_grid(noise, amplitudes_dev, tensor_rank=variable, index0=multi_index)
    with watch('transforms'):
        work.poisson_backward()
    # δ → ϱ, uⁱ → Jⁱ (ic.py:428-456), the constants as the reference hoists them
    ϱ_bar = component.ϱ_bar
    w = component.w(a=a)
    w_eff = component.w_eff(a=a)
    with watch('stores'):
        if variable == 0:
            nongaussianity = realization_options(component)['nongaussianity']
            work.fluid_from_mesh(component.ϱ, 0, ϱ_bar, nongaussianity)
        else:
            work.fluid_from_mesh(component.J[multi_index], 1, a**(1 - 3*w_eff)*ϱ_bar*(1 + w))
    watch.finish()
    return noise


def realize(component, a, amplitudes, amplitudes_θ=None, **kw):
    """Realise a component at scale factor a (realize, ic.py:297-364).  Particles go to
    realize_particles(component, a, amplitudes, amplitudes_θ, **kw).  A fluid gets ϱ and, with
    a Boltzmann order of 1 or more, J[0..2] (amplitudes_θ is then needed), all from one noise
    slab generated and uploaded once; 𝒫 = c²wϱ follows (realize_approximative,
    ic.py:495-511; w is constant here).  kw for a fluid: timings, noise_on."""
    if component.representation == 'particles':
        return realize_particles(component, a, amplitudes, amplitudes_θ, **kw)
    timings = kw.pop('timings', None)
    noise_on = kw.pop('noise_on', 'host')
    if kw:
        raise ConceptGPUError(f'{component.name}: realize() of a fluid component takes no '
                              f'{sorted(kw)}')
    with_J = component.boltzmann_order >= 1
    if with_J and amplitudes_θ is None:
        raise ConceptGPUError(f'{component.name}: J comes from the amplitudes of θ: pass '
                              'amplitudes_θ')
    noise = realize_fluid(component, a, amplitudes, 0, timings=timings, noise_on=noise_on)
    if with_J:
        for multi_index in range(3):
            realize_fluid(component, a, amplitudes_θ, 1, multi_index, noise=noise, timings=timings)
    # 𝒫 = ϱ·ℝ[light_speed**2*w] (ic.py:504-508)
    torch.mul(component.ϱ, component.params.light_speed**2*component.w(a=a), out=component.𝒫)
    return noise


# ---- the shear of closure 'class' (ic.py:471-475, 599-626, 743-762, 863-871) ------------------------
def amplitudes_from_transfer_ratio(k, ratio, gridsize, boxsize, ϱ_bar):
    """The k²-indexed table get_amplitudes makes for a variable realised from the non-linear
    structure (ic.py:599-626, use_primordial False), from a tabulated ratio of transfer functions
    T(k)/T_δ(k): amplitudes[k2] = ratio(k_f·√k2)·(gridsize**(-3)/ϱ_bar) for k2 = 1 ..
    3(nyquist-1)², the ratio interpolated linearly in log k; amplitudes[0] = 0.  The gridsize⁻³
    normalises the forward transform of ϱ, the 1/ϱ_bar turns ϱ into 1 + δ."""
    k, ratio = np.asarray(k, dtype=np.float64), np.asarray(ratio, dtype=np.float64)
    if k.ndim != 1 or k.shape != ratio.shape or k.size < 2 or np.any(np.diff(k) <= 0):
        raise ConceptGPUError('amplitudes_from_transfer_ratio(): k must be increasing, ratio of '
                              'its length')
    nyquist = int(gridsize)//2
    k2_max = 3*(nyquist - 1)**2
    k_fundamental = 2*π/boxsize
    amplitudes = np.zeros(k2_max + 1, dtype=np.float64)
    k_magnitude = k_fundamental*np.sqrt(np.arange(1, k2_max + 1, dtype=np.float64))
    if k2_max and (k_magnitude[0] < k[0] or k_magnitude[-1] > k[-1]):
        raise ConceptGPUError(
            f'amplitudes_from_transfer_ratio(): the table covers k in [{k[0]}, {k[-1]}], the grid '
            f'needs [{k_magnitude[0]}, {k_magnitude[-1]}]')
    amplitudes[1:] = np.interp(np.log(k_magnitude), np.log(k), ratio)*(
        float(gridsize)**(-3)/ϱ_bar)
    return amplitudes


def check_shear_scope(component):
    """what the realisation of ς needs of a component; fluid.py adds what the Euler equation needs"""
    name = component.name
    if component.representation != 'fluid':
        raise ConceptGPUError(f'{name}: the shear ς is a variable of fluid components')
    closure = getattr(component, 'boltzmann_closure', 'truncate')
    if closure != 'class' or component.boltzmann_order != 1:
        raise ConceptGPUError(
            f'{name}: Boltzmann closure "{closure}" with boltzmann_order = '
            f'{component.boltzmann_order}: ς is realised for closure "class" at boltzmann_order = 1 '
            '(non-linear ϱ and J) alone; a non-linear ς or 𝒫 and a linear J are not implemented')
    structure = is_selected(component, component.params.realization_options['structure'])
    if structure != 'nonlinear':
        raise ConceptGPUError(
            f'{name}: realization_options["structure"] = "{structure}": ς is realised from the '
            'component\'s own density field, select "nonlinear" for it (ς from the primordial '
            'noise is not implemented)')
    if _comm.active() is not None or getattr(component, 'nprocs', 1) > 1:
        raise ConceptGPUError(f'{name}: the realisation of ς with an active comm process group: '
                              'multi-GPU realisation is not implemented')


def fluid_structure(component, out=None):
    """ℱₓ[ϱ(x⃗)] of a fluid component (get_slab_structure, ic.py:863-871): its ϱ grid as plain
    values in a realisation mesh (`out`, or the component's own), transformed forward,
    unnormalised.  No deposit factor and no deconvolution apply.  Returns the mesh."""
    mesh = out if out is not None else _realization_mesh(component, 'realize structure')
    if mesh.gridsize != component.gridsize:
        raise ConceptGPUError(f'{component.name}: a structure mesh of grid size {mesh.gridsize} '
                              f'for a fluid of grid size {component.gridsize}')
    mesh.fluid_add(component.ϱ, 1.0, '=')
    mesh.fft_forward()
    return mesh


def realize_shear(component, a, amplitudes, multi_index=(0, 0), structure=None, out=None):
    """ςₘₙ of a fluid component with closure 'class' at scale factor a (realize_fluid with
    variable 2, ic.py:400-475, the non-compound case), realised from the component's own
    non-linear density: amplitudes[k²]·(½δₘₙ - (3/2)kₘkₙ/k²)·ℱ[ϱ], back to real space, times
    ϱ_bar(1 + w).  The inspection and test path: the time loop forms the divergence of ς in
    Fourier space without the six grids (fluid.shear_sources).

    amplitudes: the k²-indexed table of σ (amplitudes_from_transfer_ratio).
    structure: the mesh fluid_structure() returned, to realise several elements from one
      transform of ϱ.
    out: a (gridsize, gridsize, gridsize) device tensor to receive ςₘₙ; it is not stored on the
      component.  Returns it."""
    check_shear_scope(component)
    try:
        index0, index1 = (int(i) for i in multi_index)
    except (TypeError, ValueError):
        index0 = index1 = -1
    if not (0 <= index0 < 3 and 0 <= index1 < 3):
        raise ConceptGPUError(f'{component.name}: realize_shear() needs a multi_index (m, n) with '
                              f'm, n in {{0, 1, 2}}, not {multi_index!r}')
    gridsize = component.gridsize
    amplitudes_dev = _amplitudes_dev(component, amplitudes, gridsize, 'a fluid grid of {}³ cells')
    if structure is None:
        structure = fluid_structure(component)
    if out is None:
        out = torch.empty_like(component.ϱ)
    work = _realization_mesh(component, 'realize work')
    work.realize_grid_tensor(structure, amplitudes_dev, index0, index1)
    work.poisson_backward()
    # σⁱⱼ → ςⁱⱼ ≈ ϱ_bar(1 + w)σⁱⱼ (ic.py:471-475)
    return work.fluid_from_mesh(out, 1, component.ϱ_bar*(1 + component.w(a=a)))


def _amplitudes_dev(component, amplitudes, gridsize, what='a lattice of {}³ particles'):
    amplitudes = np.ascontiguousarray(np.asarray(amplitudes, dtype=np.float64))
    k2_max = 3*(gridsize//2 - 1)**2
    if amplitudes.shape != (k2_max + 1,):
        raise ConceptGPUError(
            f'{component.name}: {amplitudes.shape} amplitudes for {what.format(gridsize)}, '
            f'which needs 3*(nyquist - 1)**2 + 1 = {k2_max + 1}')
    return torch.from_numpy(amplitudes).to(component.device)


@contextlib.contextmanager
def _host_timer(timings, kind):
    import time
    t0 = time.perf_counter()
    yield
    if timings is not None:
        timings[kind] = timings.get(kind, 0.0) + (time.perf_counter() - t0)*1e3
