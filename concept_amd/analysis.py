"""concept_amd.analysis — power spectra of the components (the reference's analysis.py).

  powerspec()                    analysis.py:70-93
  get_powerspec_declarations()   analysis.py:118-197 with get_output_declarations
                                 (graphics.py:1080-1143)
  get_powerspec_bins()           analysis.py:235-438, construct_powerspec_k_bin_centers
                                 analysis.py:441-496
  compute_powerspec()            analysis.py:500-579: interpolate_upstream(..., 'ρ', ...,
                                 output_space='Fourier') (mesh.py:492-635; here
                                 interactions.interpolate_upstream, the one gravity uses) on
                                 mesh contexts of their own roles, then the k-shell binning in
                                 HIP (cg_powerspec_bin, csrc/cg_analysis.hip)
  compute_powerspec_σ()          analysis.py:856-914
  save_powerspec()               analysis.py:796-833 with save_polyspec / get_txt_info
                                 (analysis.py:3283-3484, 3495-3751)
The linear and corrected spectra need CLASS, and plots need matplotlib: a selection that asks
for them is warned about once and left out; 'data' is what gets computed.

The bispectrum's computational core:
  compute_bispec_value()         analysis.py:2576-2707 with get_bispec_grid (2739-2789): shell
                                 fields and triple sums in HIP (cg_bispec_shell,
                                 cg_bispec_sums, csrc/cg_bispec.hip)
  bispec_measure()               compute_bispec (analysis.py:3031-3166) and the mode counting
                                 of get_bispec_bins (analysis.py:1293-1316) for explicit bins
The configuration grammar, the shell boundaries, the tree-level bispectrum, the file, the
dump of the time loop, plots and the on-disk mode cache are not built.

Conservation and shock diagnostics:
  measure()                      analysis.py:3860-4230: 'v_max', 'v_rms', 'momentum', 'ϱ', 'mass'
                                 and 'discontinuity' of a particle or fluid component; the sums
                                 in double-double on the GPU (cg_measure_sums,
                                 cg_measure_fluid_velocity, cg_measure_discontinuity,
                                 csrc/cg_measure.hip) and finished in decimal by combine_sums()
The utility info --stats and decaying species (w_eff ≠ w) are not built."""
import collections
import decimal
import hashlib
import itertools
import math
import os
import re
import warnings

import numpy as np
import torch

from . import commons
from . import comm as _comm
from .interactions import interpolate_upstream
from .lib import ConceptGPUError, _ptr, check, raw
from .mesh import get_mesh

π = commons.π

PowerspecDeclaration = collections.namedtuple(
    'PowerspecDeclaration',
    ('components', 'do_data', 'do_corrected', 'do_linear', 'do_plot', 'gridsize',
     'interpolation', 'deconvolve', 'interlace', 'realization_correction', 'k2_max', 'k_max',
     'bins_per_decade', 'tophat', 'significant_figures', 'k_bin_indices', 'k_bin_centers',
     'n_modes', 'power', 'power_corrected', 'power_linear'),
    defaults=[None]*21)

_unsupported_warned = set()
powerspec_declarations_cache = {}
powerspec_bins_cache = {}
_device_tables = {}


# -- selections (commons.py:5471-5600 for several components) ----------------------------------
def is_selected(components, d, default=None):
    """is_selected for one component (commons.is_selected) or for a combination: then keys are
    'default', 'all combinations' and collections of representations, species or names."""
    components = list(components) if isinstance(components, (list, tuple)) else [components]
    if len(components) == 1:
        return commons.is_selected(components[0], d, default=default)
    names = frozenset(c.name.lower() for c in components)
    representations = frozenset(c.representation.lower() for c in components)
    single_species = frozenset(s_.lower() for c in components for s_ in c.species.split('+'))
    species = frozenset(c.species.lower() for c in components)
    keys = ('default', 'all combinations', representations, single_species, species, names)
    lowered = {}
    for key, val in d.items():
        if isinstance(key, str):
            key = key.lower()
        else:
            key = [k.lower() if isinstance(k, str) else getattr(k, 'name', str(k)).lower()
                   for k in key]
            if not key:
                continue
            key = key[0] if len(key) == 1 else frozenset(key)
        lowered[key] = val
    found = [lowered[k] for k in keys if k in lowered]
    return found[-1] if found else default


def _eval_expr(expr, mapping):
    """eval_bin_str (analysis.py:470-494) / to_float: a string expression of the names in
    `mapping` and the units"""
    if not isinstance(expr, str):
        return float(expr)
    p = commons.params
    ns = {'sqrt': math.sqrt, 'cbrt': np.cbrt, 'log': math.log, 'log10': math.log10, 'exp': math.exp,
          'π': π, 'pi': π, 'min': min, 'max': max}
    if p is not None:
        ns.update(vars(p.units))
    full = {}
    for key, val in mapping.items():
        base = key[2:] if key.startswith('k_') else key
        for k in (base, base.lower(), base.capitalize()):
            for k2 in (f'k_{k}', f'k{k}', k, k.replace('_', '')):
                if k2 not in ('min', 'max'):   # (the functions keep their names)
                    full[k2] = val
    ns.update(full)
    return float(eval(expr, {}, ns))


def upstream_gridsize(component, output_type='powerspec'):
    """Component.<output_type>_upstream_gridsize (species.py:1371-1394) for the output types
    'powerspec' and 'render2D': the selected 'upstream gridsize', else 2*cbrt(Ñ) for particles
    and the fluid's own grid size for fluids."""
    p = commons.params
    # (bispec_options is not read: the bispectrum takes the reference's default here)
    options = getattr(p, f'{output_type}_options', None) or {'upstream gridsize': {}}
    g = is_selected(component, options['upstream gridsize'], default=-1)
    if g == -1:
        g = 'gridsize' if component.representation == 'fluid' else '2*cbrt(Ñ)'
    if isinstance(g, str):
        N = component.N if component.representation == 'particles' else component.gridsize**3
        g = _eval_expr(g, {'Ñ': N, 'N': N, 'gridsize': getattr(component, 'gridsize', -1) or -1})
    g = int(round(float(g)))
    if component.representation == 'fluid' and g != component.gridsize:
        raise ConceptGPUError(
            f'{component.name}: '
            f'{ {"powerspec": "power spectrum", "bispec": "bispectrum"}.get(output_type, output_type)} '
            f'upstream grid size {g} differs from the fluid '
            f'grid size {component.gridsize}')
    return g


# -- declarations ------------------------------------------------------------------------------
def get_output_declarations(output_type, components, selections, options):
    """The generic part of the output declarations (graphics.py:1080-1143), for the output types
    'powerspec' and 'render2D': for every combination of components for which `selections`
    selects at least one output, (combination, {output: bool}, specifications).  The
    specifications are the options looked up for the combination under their names with '_'
    for ' ', and 'gridsize': the 'global gridsize', or the largest upstream grid size of the
    combination where that is -1."""
    combinations = itertools.chain.from_iterable(
        itertools.combinations(components, i) for i in range(1, len(components) + 1))
    for combination in map(list, combinations):
        do = {key: bool(is_selected(combination, {k: v[key] for k, v in selections.items()},
                                    default=False))
              for key in selections['default']}
        if not any(do.values()):
            continue
        gridsize = is_selected(combination, options['global gridsize'], default=-1)
        if gridsize == -1:
            gridsize = max(upstream_gridsize(c, output_type) for c in combination)
        specifications = {'gridsize': int(gridsize)}
        specifications.update({key.replace(' ', '_'): is_selected(combination, option)
                               for key, option in options.items()
                               if key not in ('upstream gridsize', 'global gridsize')})
        yield combination, do, specifications


def get_powerspec_declarations(components):
    """One declaration per component combination that powerspec_select selects (graphics.py:
    1080-1143), with the bins of get_powerspec_bins.  'linear', 'corrected' (need CLASS) and
    'plot' are warned about once and switched off; what remains of a selection computes
    'data'."""
    p = commons.params
    cache_key = (id(p),) + tuple(id(c) for c in components)
    declarations = powerspec_declarations_cache.get(cache_key)
    if declarations:
        return declarations
    declarations = []
    for combination, do, spec in get_output_declarations(
            'powerspec', components, p.powerspec_select, p.powerspec_options):
        gridsize = spec.pop('gridsize')
        for key, why in (('linear', 'needs CLASS'), ('corrected', 'needs CLASS'),
                         ('plot', 'plots are not produced')):
            if do[key] and key not in _unsupported_warned:
                _unsupported_warned.add(key)
                warnings.warn(f"powerspec_select: '{key}' {why}; it is left out")
        k2_max, k_bin_indices, k_bin_centers, n_modes = get_powerspec_bins(
            int(gridsize), spec['k_max'], spec['bins_per_decade'])
        declarations.append(PowerspecDeclaration(
            components=combination, do_data=True, do_corrected=False, do_linear=False,
            do_plot=False, gridsize=int(gridsize), k2_max=k2_max, k_bin_indices=k_bin_indices,
            k_bin_centers=k_bin_centers, n_modes=n_modes,
            power=np.empty(len(k_bin_centers)), **spec))
    powerspec_declarations_cache[cache_key] = declarations
    return declarations


# -- bins --------------------------------------------------------------------------------------
def _controlpoint_spline(d):
    """get_controlpoint_spline(d, np.log10) (commons.py:5436-5465): linear in log10 of the
    keys, clamped at the ends; looked up with log10 k"""
    x = np.log10(np.fromiter(d.keys(), dtype=np.float64))
    y = np.fromiter(d.values(), dtype=np.float64)
    order = np.argsort(x, kind='stable')
    x, y = x[order], y[order]
    return lambda logk: float(np.interp(logk, x, y))


def construct_powerspec_k_bin_centers(k_min, k_max, bins_per_decade, gridsize, nyquist):
    """analysis.py:441-496"""
    k_fundamental = 2*π/commons.params.boxsize
    binsize_min = (0.5*(1 - 1e-2)*k_fundamental
                   * (math.sqrt(3*nyquist**2 + 1) - math.sqrt(3*nyquist**2)))
    mapping = {'nyquist': k_fundamental*nyquist, 'gridsize': gridsize, 'k_min': k_min,
               'k_max': k_max, 'k_fundamental': k_min, 'k_f': k_min}
    bpd = {}
    for k, val in bins_per_decade.items():
        bpd[_eval_expr(k.strip(), mapping) if isinstance(k, str) else k] = (
            _eval_expr(val, mapping) if isinstance(val, str) else val)
    if len(bpd) == 1:
        bpd.update({k + 1: val for k, val in bpd.items()})
    logk_min, logk_max = math.log10(k_min), math.log10(k_max)
    interp = _controlpoint_spline(bpd)
    centers = []
    logk_bin_right = logk_min - 0.5/interp(logk_min)
    while logk_bin_right <= logk_max:
        logk_bin_left = logk_bin_right
        logk_bin_right = logk_bin_left + 1/interp(logk_bin_left)
        logk_bin_right = np.max((logk_bin_right, math.log10(10**logk_bin_left + binsize_min)))
        centers.append(10**(0.5*(logk_bin_left + logk_bin_right)))
    if not centers:
        centers.append(math.sqrt(k_min*k_max))
    centers = np.asarray(centers, dtype=np.float64)
    if len(centers) > 1:
        left = k_min
        right = 10**(logk_max - 0.5/interp(logk_max))
        centers = 10**(
            math.log10(left) + (np.log10(centers) - math.log10(centers[0]))*(
                (math.log10(right) - math.log10(left))
                / (math.log10(centers[-1]) - math.log10(centers[0]))))
    return centers


def n_modes_per_k2(gridsize, k2_max):
    """The multiplicity of every k² in [0, k2_max] over fourier_loop(gridsize, sparse=True,
    skip_origin=True, k2_max) (mesh.py:2748-2838), in closed form: the (ki, kj) pairs off the
    Nyquist planes by ki² + kj², shifted by every kk² with 0 < kk < nyquist, plus half of the
    kk = 0 plane (one of each conjugate pair, the origin left out).  Cached per
    (gridsize, k2_max)."""
    key = ('n_modes', int(gridsize), int(k2_max))
    n = powerspec_bins_cache.get(key)
    if n is not None:
        return n
    N, nyq = int(gridsize), int(gridsize)//2
    a = np.array([i for i in range(N) if i != nyq], dtype=np.int64)
    k1 = a - np.where(a >= nyq, N, 0)
    ki, kj = np.meshgrid(k1, k1, indexing='ij')
    s = (kj**2 + ki**2).ravel()
    keep = s <= k2_max
    c2 = np.bincount(s[keep], minlength=k2_max + 1)[:k2_max + 1]
    plane0 = ~((ki > 0) | ((ki == 0) & (kj >= 0))).ravel()
    n = np.bincount(s[keep & plane0], minlength=k2_max + 1)[:k2_max + 1].astype(np.int64)
    for kk in range(1, nyq):
        shift = kk*kk
        if shift > k2_max:
            break
        n[shift:] += c2[:k2_max + 1 - shift]
    powerspec_bins_cache[key] = n
    return n


def get_powerspec_bins(gridsize, k_max, bins_per_decade):
    """analysis.py:235-438: (k2_max, k_bin_indices, k_bin_centers, n_modes)."""
    p = commons.params
    cache_key = (gridsize, p.boxsize, k_max, tuple(bins_per_decade.items()))
    bins = powerspec_bins_cache.get(cache_key)
    if bins:
        return bins
    k_fundamental = 2*π/p.boxsize
    k_min = k_fundamental
    nyquist = gridsize//2
    if isinstance(k_max, str):
        k_max = _eval_expr(k_max, {'nyquist': k_fundamental*nyquist, 'gridsize': gridsize,
                                   'k_min': k_min, 'k_fundamental': k_min, 'k_f': k_min})
    if k_max < k_min:
        warnings.warn(f'Power spectrum k_max was set to {k_max} < k_min = 2π/boxsize = '
                      f'{k_min}. Setting k_max = k_min.')
        k_max = k_min
    k2_max = int(round((k_max/k_fundamental)**2))
    k2_max = min(k2_max, 3*nyquist**2)
    k_max = k_fundamental*math.sqrt(k2_max)
    k_bin_centers = construct_powerspec_k_bin_centers(k_min, k_max, bins_per_decade, gridsize,
                                                      nyquist)
    logk_bin_centers = np.log(k_bin_centers)
    k2 = np.arange(1, k2_max + 1)
    logk = np.log(k_fundamental*np.sqrt(k2.astype(np.float64)))
    index = np.searchsorted(logk_bin_centers, logk)
    nb = k_bin_centers.shape[0]
    last = index == nb
    mid = (~last) & (index != 0)
    im = index[mid]
    dist_left = logk[mid] - logk_bin_centers[im - 1]
    dist_right = logk_bin_centers[im] - logk[mid]
    index[mid] = im - (dist_left <= dist_right)
    index[last] -= 1
    k_bin_indices = np.empty(k2_max + 1, dtype=np.int64)
    k_bin_indices[0] = 0
    k_bin_indices[1:] = index
    n_modes_fine = n_modes_per_k2(gridsize, k2_max)
    # centres: the mode-weighted geometric mean of the k that fall into a bin
    occupied = np.nonzero(n_modes_fine[1:])[0] + 1
    bins_occ = k_bin_indices[occupied]
    n_modes = np.bincount(bins_occ, weights=n_modes_fine[occupied], minlength=nb).astype(np.int64)
    log_sum = np.zeros(nb)
    for b, w in zip(bins_occ, n_modes_fine[occupied]*np.log(
            k_fundamental*np.sqrt(occupied.astype(np.float64)))):
        log_sum[b] += w
    k_bin_centers = np.zeros(nb)
    filled = n_modes > 0
    k_bin_centers[filled] = np.exp(log_sum[filled]/n_modes[filled])
    # consecutive indices for the non-empty bins (k_bin_indices never decreases along k²)
    rank = np.cumsum(filled) - 1
    new = np.where(filled[k_bin_indices], rank[k_bin_indices], -1)
    new[0] = 0
    k_bin_indices = np.maximum.accumulate(new)
    bins = (k2_max, k_bin_indices, k_bin_centers[filled], n_modes[filled])
    powerspec_bins_cache[cache_key] = bins
    return bins


# -- the spectrum ------------------------------------------------------------------------------
def _mesh(gridsize, role):
    p = commons.params
    return get_mesh(gridsize, p.boxsize, p.nghosts, p.cell_centered, 2, None, role=role)


def _device_bin_table(declaration, device):
    key = (id(declaration.k_bin_indices), str(device))
    t = _device_tables.get(key)
    if t is None:
        t = _device_tables[key] = torch.from_numpy(
            np.ascontiguousarray(declaration.k_bin_indices, dtype=np.int32)).to(device)
    return t


def compute_powerspec(declaration, a=1.0, timings=None):
    """analysis.py:500-579: the binned power of the declaration's components into
    declaration.power (on every rank; under comm.init() the ranks' partial bins are summed in
    rank order).  timings: a dict that receives the seconds of the upstream interpolation
    (deposits and FFTs) and of the binning."""
    components = declaration.components
    gridsizes_upstream = [upstream_gridsize(c) for c in components]
    if timings is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
    # quantity 'ρ' (mesh.py:1543-1549, 1713-1718)
    slab = interpolate_upstream(components, gridsizes_upstream, declaration.gridsize,
                                lambda c: a**(-3*(1 + c.w_eff(a=a))), declaration.interpolation,
                                declaration.deconvolve, declaration.interlace,
                                roles=('powerspec', 'powerspec upstream'))
    if timings is not None:
        ev[1].record()
    nbins = len(declaration.k_bin_centers)
    power = slab.powerspec_bin(_device_bin_table(declaration, slab.device),
                               declaration.k2_max, nbins)
    if timings is not None:
        ev[2].record()
        ev[2].synchronize()
        timings['upstream'] = ev[0].elapsed_time(ev[1])*1e-3
        timings['binning'] = ev[1].elapsed_time(ev[2])*1e-3
    power = power.cpu().numpy()
    c = _comm.active()
    if c is not None and c.world > 1:
        power = c.sum_in_rank_order(power)
    # normalisation (analysis.py:567-577)
    normalization = 0
    for component in components:
        normalization += a**(-3*(1 + component.w_eff(a=a)))*component.ϱ_bar
    normalization **= -2
    normalization *= commons.params.boxsize**3
    power = power*(normalization/declaration.n_modes)
    declaration.power[:] = power
    return declaration.power


def compute_powerspec_σ(declaration, kind='data'):
    """analysis.py:856-914: the rms density variation in a sphere of radius tophat"""
    kind = kind.lower().replace(' ', '').replace('-', '').replace('_', '')
    if kind != 'data':
        raise ConceptGPUError(f'compute_powerspec_σ() called with kind = "{kind}": only "data" '
                              'spectra are computed here (the others need CLASS)')
    tophat = declaration.tophat
    k = np.asarray(declaration.k_bin_centers, dtype=np.float64)
    power = np.asarray(declaration.power, dtype=np.float64)
    mask = np.isnan(power)
    if mask.any():
        power, k = power[~mask], k[~mask]
    if k.shape[0] < 2:
        return float('nan')
    kR = k*tophat
    with np.errstate(invalid='ignore', divide='ignore'):
        W = np.where(kR < 1e-3, 1./3. - 1./30.*kR**2, (np.sin(kR) - kR*np.cos(kR))/kR**3)
    integrand = (k*W)**2*power
    σ2 = float(np.trapezoid(integrand, k) if hasattr(np, 'trapezoid') else np.trapz(integrand, k))
    σ2 += 0.5*k[0]*integrand[0]
    σ2 *= 3**2/(2*π**2)
    return math.sqrt(σ2)


# -- the file ----------------------------------------------------------------------------------
_subscripts = dict(zip('0123456789-+.e', '₀₁₂₃₄₅₆₇₈₉₋₊.ₑ'))


def unicode_subscript(s):
    return ''.join(_subscripts.get(ch, ch) for ch in s)


def _components_str(components):
    s = ', '.join(c.name for c in components)
    return f'{{{s}}}' if len(components) > 1 else s


def save_powerspec(declarations, filename, a=None, t=None):
    """save_powerspec (analysis.py:796-833) through save_polyspec (analysis.py:3283-3484):
    a header (time, components with their upstream grid sizes, per column group the global grid
    size and every declaration's σ line), then one column group per binning — k, modes and the
    P of each declaration of that binning — floats as %.{sf-1}e, shorter columns padded with
    NaN.  Only rank 0 writes."""
    p = commons.params
    c = _comm.active()
    if c is not None and c.rank != 0:
        return filename
    declarations = [d for d in declarations if d.do_data]
    if not declarations:
        return filename
    sf = max(int(d.significant_figures) for d in declarations)
    σ_unit = p.units.Mpc/(p.H0/(100*p.units.km/(p.units.s*p.units.Mpc))) if p.enable_Hubble \
        else p.units.Mpc
    groups = collections.OrderedDict()
    for d in declarations:
        key = (len(d.k_bin_centers), d.k2_max,
               hashlib.sha1(np.ascontiguousarray(d.k_bin_centers)).hexdigest())
        groups.setdefault(key, []).append(d)
    lines = []
    tline = f'Power spectra at t = {t:.{sf}g} Gyr' if t is not None else 'Power spectra'
    if p.enable_Hubble and a is not None:
        tline += f', a = {a:.{sf}g}'
    lines.append(tline + ', computed with:')
    comps = []
    for d in declarations:
        for comp in d.components:
            if comp not in comps:
                comps.append(comp)
    width = max(len(comp.name) for comp in comps)
    lines.append(f'  {"component":<{width}}  upstream gridsize')
    for comp in comps:
        lines.append(f'  {comp.name:<{width}}  {upstream_gridsize(comp)}')
    columns, headings = [], []
    for gi, ((nbins, k2_max, _), group) in enumerate(groups.items()):
        d0 = group[0]
        lines.append(f'Column group {gi + 1}: global gridsize {d0.gridsize}, '
                     f'k_max = {math.sqrt(k2_max)*2*π/p.boxsize:.{sf}g} Mpc⁻¹')
        for d in group:
            σ = compute_powerspec_σ(d)
            sub = unicode_subscript(f'{d.tophat/σ_unit:.3g}')
            lines.append(f'  {_components_str(d.components)}: σ{sub} = {σ:.{sf - 1}e}')
        columns.append(('k', np.asarray(d0.k_bin_centers, dtype=np.float64)))
        headings.append('k [Mpc⁻¹]')
        columns.append(('modes', np.asarray(d0.n_modes)))
        headings.append('modes')
        for d in group:
            columns.append(('P', np.asarray(d.power, dtype=np.float64)))
            headings.append(f'P [Mpc³] {_components_str(d.components)}')
    nrows = max(len(col) for _, col in columns)
    fw = sf + 6
    lines.append('  '.join(f'{h:<{fw}}' for h in headings).rstrip())
    body = []
    for r in range(nrows):
        cells = []
        for kind, col in columns:
            if r >= len(col):
                cells.append(f'{"nan":<{fw}}')
            elif kind == 'modes':
                cells.append(f'{int(col[r]):<{fw}d}')
            else:
                cells.append(f'{col[r]:<{fw}.{sf - 1}e}')
        body.append('  '.join(cells).rstrip())
    d = os.path.dirname(filename)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(filename, 'w', encoding='utf-8') as f:
        f.write('\n'.join('# ' + line for line in lines) + '\n')
        f.write('\n'.join(body) + '\n')
    return filename


def powerspec(components, filename, a=1.0, t=None, timings=None):
    """analysis.py:70-93: compute the power spectra that powerspec_select asks for and write
    them to `filename`.  a: the current scale factor (universals.a)."""
    declarations = get_powerspec_declarations(components)
    for declaration in declarations:
        compute_powerspec(declaration, a, timings)
    save_powerspec(declarations, filename, a, t)
    return declarations


def load_powerspec_σ(filename, tophat_Mpc):
    """The σ of the first declaration from a written file, found the way the reference's
    test/powerspec/analyze.py does (regex on the header)."""
    with open(filename, encoding='utf-8') as f:
        for line in f:
            m = re.search('σ' + unicode_subscript(f'{tophat_Mpc:.2g}') + r' = ([0-9\.e+-]*)', line)
            if m:
                return float(m.group(1))
    return None


# -- the bispectrum: the computational core (analysis.py:929-3280) ------------------------------
BispecResult = collections.namedtuple(
    'BispecResult', ('n_modes', 'bpower', 'power', 'bpower_reduced', 'n_modes_power'))

# compute_bispec_value's three grids of the previous call: (shell, gridsize, is_indicator) ->
# (buffer number, mesh)  (analysis.py:2708-2710)
bispec_grid_cache = {}
_bispec_cache_antialiasing = [None]


def _bispec_antialiasing(antialiasing):
    if antialiasing is not None:
        return bool(antialiasing)
    return bool(getattr(commons.params, 'bispec_antialiasing', True))


def get_bispec_grid(gridsize, shell, buffer_number, slab_data, antialiasing):
    """get_bispec_grid (analysis.py:2739-2789): the shell-filtered copy of slab_data's Fourier
    view (the indicator field of the shell without slab_data) on the mesh of role
    'bispec <buffer_number>', transformed back to real space."""
    grid = _mesh(gridsize, f'bispec {buffer_number}')
    grid.bispec_shell(shell, slab_data, antialiasing)
    grid.poisson_backward()
    return grid


def _bispec_sums(grids, power_mask):
    """(value, Σg₀², Σg₁², Σg₂²) of this rank's layers as floats"""
    return grids[0].bispec_sums(grids[1:], power_mask).cpu().tolist()


def compute_bispec_value(gridsize, shells, power_dict, slab_data=None, *, antialiasing=None):
    """compute_bispec_value (analysis.py:2576-2707), the Scoccimarro estimator: the sum over
    the cells of the product of the three shell-filtered grids.  shells: three (k_inner,
    k_outer) in grid units.  Without slab_data (the mesh whose Fourier view holds the data)
    the grids are indicator fields and (value, shells_new) is returned, else the value.
    power_dict (or None) receives Σ grid² under every shell it does not hold yet.  The value
    is unnormalised and of this rank's layers only: under comm.init() the caller combines the
    ranks with sum_in_rank_order.  A grid is reused when the previous call built it for the
    same (shell, gridsize, is_indicator)."""
    antialiasing = _bispec_antialiasing(antialiasing)
    if _bispec_cache_antialiasing[0] != antialiasing:
        bispec_grid_cache.clear()
        _bispec_cache_antialiasing[0] = antialiasing
    shells = [tuple(float(k) for k in shell) for shell in shells]
    if len(shells) != 3:
        raise ConceptGPUError(f'compute_bispec_value(): {len(shells)} shells given, not 3')
    is_indicator = slab_data is None
    shellinfos_counter = collections.Counter((shell, int(gridsize), is_indicator)
                                             for shell in shells)
    # grids of the previous call first, then the ones to build (analysis.py:2599-2617)
    shellinfos, gridinfos = [], []
    buffer_numbers = {0, 1, 2}
    for shellinfo, multiplicity in shellinfos_counter.items():
        loot = bispec_grid_cache.get(shellinfo)
        if loot is not None:
            shellinfos.append(shellinfo)
            n, grid = loot
            gridinfos.append((multiplicity, n, grid))
            buffer_numbers -= {n}
    for shellinfo, multiplicity in shellinfos_counter.items():
        if shellinfo not in bispec_grid_cache:
            shellinfos.append(shellinfo)
            n = min(buffer_numbers)
            buffer_numbers -= {n}
            grid = get_bispec_grid(int(gridsize), shellinfo[0], n, slab_data, antialiasing)
            gridinfos.append((multiplicity, n, grid))
    if len(gridinfos) == 2 and gridinfos[0][0] > gridinfos[1][0]:
        # Σ g₀g₁²: the grid that counts twice is grid 1 (analysis.py:2656-2658)
        gridinfos.reverse()
        shellinfos.reverse()
    unique_shells = [shellinfo[0] for shellinfo in shellinfos]
    compute_power = [power_dict is not None and shell not in power_dict
                     for shell in unique_shells]
    power_mask = sum(1 << q for q, want in enumerate(compute_power) if want)
    sums = _bispec_sums([grid for _, _, grid in gridinfos], power_mask)
    value = sums[0]
    shells_new = []
    for q, (shell, want) in enumerate(zip(unique_shells, compute_power)):
        if want:
            power_dict[shell] = sums[1 + q]
            shells_new.append(shell)
    bispec_grid_cache.clear()
    for shellinfo, (_, n, grid) in zip(shellinfos, gridinfos):
        bispec_grid_cache[shellinfo] = (n, grid)
    return (value, shells_new) if is_indicator else value


def _sum_ranks(values):
    values = np.asarray(values, dtype=np.float64)
    c = _comm.active()
    if c is not None and c.world > 1 and values.size:
        values = c.sum_in_rank_order(values)
    return values


def bispec_measure(components, shells_per_bin, gridsize, *, interpolation='PCS', deconvolve=True,
                   interlace=True, do_reduced=True, a=1.0, antialiasing=None):
    """compute_bispec (analysis.py:3031-3166) with the mode-counting half of get_bispec_bins
    (analysis.py:1293-1316) for an explicit list of bins, each a triple of (k_inner, k_outer)
    shells in grid units, processed in the given order.  Returns a BispecResult of arrays:
    n_modes and bpower [boxsize⁶] per bin, power [boxsize³] (3 x nbins, the bin's shells in
    the given order), bpower_reduced = B/(P₁P₂ + P₂P₃ + P₃P₁), and n_modes_power
    (3 x nbins).  Empty bins and shells give NaN.  power and bpower_reduced are NaN without
    do_reduced.  Collective under comm.init(); every rank returns the full result."""
    antialiasing = _bispec_antialiasing(antialiasing)
    gridsize = int(gridsize)
    bins = [tuple(tuple(float(k) for k in shell) for shell in shells)
            for shells in shells_per_bin]
    nbins = len(bins)
    order = int(commons.interpolation_orders.get(str(interpolation).upper(), interpolation))
    lattice = commons._interlace2latticekind(interlace)
    # the mode counts (analysis.py:1293-1316): indicator fields, normalised by 0.5/N³
    bispec_grid_cache.clear()
    normalization = 0.5/gridsize**3
    n_modes = np.zeros(nbins)
    n_modes_power = {}
    for b, shells in enumerate(bins):
        n_modes[b], _ = compute_bispec_value(gridsize, shells, n_modes_power,
                                             antialiasing=antialiasing)
    n_modes = _sum_ranks(n_modes)*normalization
    n_modes_power = dict(zip(n_modes_power,
                             _sum_ranks(list(n_modes_power.values()))*normalization))
    # the data (analysis.py:3056-3093)
    gridsizes_upstream = [upstream_gridsize(c, 'bispec') for c in components]
    slab = interpolate_upstream(components, gridsizes_upstream, gridsize,
                                lambda c: a**(-3*(1 + c.w_eff(a=a))), order, deconvolve,
                                lattice, roles=('bispec', 'bispec upstream'))
    bispec_grid_cache.clear()
    power_dict = {} if do_reduced else None
    bpower = np.zeros(nbins)
    for b, shells in enumerate(bins):
        bpower[b] = compute_bispec_value(gridsize, shells, power_dict, slab,
                                         antialiasing=antialiasing)
    bispec_grid_cache.clear()
    bpower = _sum_ranks(bpower)
    if do_reduced:
        power_dict = dict(zip(power_dict, _sum_ranks(list(power_dict.values()))))
    # normalisation (analysis.py:3097-3141)
    ρ_bar = 0
    for component in components:
        ρ_bar += a**(-3*(1 + component.w_eff(a=a)))*component.ϱ_bar
    boxsize = commons.params.boxsize
    normalization = ρ_bar**-3*(0.5*boxsize**6)/gridsize**3
    with np.errstate(divide='ignore', invalid='ignore'):
        bpower = np.where(n_modes != 0, bpower*(normalization/n_modes), np.nan)
    power = np.full((3, nbins), np.nan)
    modes_power = np.array([[n_modes_power[shell] for shell in shells] for shells in bins]
                           ).reshape(nbins, 3).T
    bpower_reduced = np.full(nbins, np.nan)
    if do_reduced:
        normalization = ρ_bar**-2*(0.5*boxsize**3)/gridsize**3
        for shell in power_dict:
            n_mode_power = n_modes_power[shell]
            power_dict[shell] = (power_dict[shell]*(normalization/n_mode_power)
                                 if n_mode_power != 0 else float('nan'))
        # the reduced bispectrum (analysis.py:3143-3164)
        for b, shells in enumerate(bins):
            power[:, b] = [power_dict[shell] for shell in shells]
        bpower_reduced = bpower/(power[0]*power[1] + power[1]*power[2] + power[2]*power[0])
    return BispecResult(n_modes=n_modes, bpower=bpower, power=power,
                        bpower_reduced=bpower_reduced, n_modes_power=modes_power)


# -- measure (analysis.py:3860-4230) -----------------------------------------------------------
MeasuredSums = collections.namedtuple('MeasuredSums', ('sum', 'sigma', 'mean', 'min', 'max_abs'))
# the numbers cg_measure_sums leaves per column: Σx (hi, lo), Σx² (hi, lo), min x, max |x|
SUMS_PER_COLUMN = 6


def combine_sums(partials, count, scale=1.0):
    """The end of a reduction of measure(), on the host: `partials` holds the six numbers of
    cg_measure_sums for one column from every domain (shape (domains, 6), or (6,) for one), in
    domain order; `count` is the number of values over all domains; `scale` multiplies every value
    (Vcell for the momentum of a fluid cell).  Returns MeasuredSums: the sum, the standard
    deviation sqrt(Σx²/count - (Σx/count)²) (a negative variance counts as 0) and the mean as the
    reference computes them in decimal with 34 digits (analysis.py:4031-4056, 4066-4090), rounded to
    double at the end, and the extremes.  A domain without values contributes 0, 0, 0, 0, +inf, 0.
    A NaN or an infinity in the sums is passed on in floating point (decimal would refuse the
    compare)."""
    partials = np.asarray(partials, dtype=np.float64).reshape(-1, SUMS_PER_COLUMN)
    x_min = float(np.min(partials[:, 4])) if partials.shape[0] else math.inf
    x_max = float(np.max(partials[:, 5])) if partials.shape[0] else 0.0
    if not np.all(np.isfinite(partials[:, :4])):
        with np.errstate(invalid='ignore'):
            total = float(np.sum(partials[:, 0]))*scale
        mean = total/count if count else math.nan
        return MeasuredSums(total, math.nan, mean, x_min, x_max)
    with decimal.localcontext() as ctx:
        ctx.prec = 2*17
        D = decimal.Decimal
        Σ = Σ2 = D(0)
        for hi, lo, hi2, lo2 in partials[:, :4].tolist():
            Σ += D(hi)
            Σ += D(lo)
            Σ2 += D(hi2)
            Σ2 += D(lo2)
        Σ *= D(scale)
        Σ2 *= D(scale)**2
        if count == 0:
            return MeasuredSums(float(Σ), math.nan, math.nan, x_min, x_max)
        mean = Σ/count
        σ2 = Σ2/count - mean**2
        σ = D(0) if σ2 < 0 else σ2.sqrt()
        return MeasuredSums(float(Σ), float(σ), float(mean), x_min, x_max)


def fluidscalar_names(component):
    """(name, grid) of the fluid scalars iterate_fluidscalars (species.py:3570-3578) yields for
    the component, in its order and with the names str(fluidscalar) gives (species.py:427-431:
    '<fluidscalar varnum[multi_index]>').  𝒫 lives on ς as its trace and is a FluidScalar(0, 0)
    (species.py:1718): it carries the name of ϱ."""
    order, closure = component.boltzmann_order, component.boltzmann_closure
    if closure != 'truncate' or order > 1:
        raise ConceptGPUError(
            f'{component.name}: measure(): quantity "discontinuity" with boltzmann_order = {order} '
            f'and Boltzmann closure "{closure}" is not implemented: the linear fluid variable of '
            'closure "class" and the ς of boltzmann_order > 1 are not kept as grids')
    scalars = [('<fluidscalar 0[0]>', component.ϱ)]
    if order == 1:
        scalars += [(f'<fluidscalar 1[{dim}]>', component.J[dim]) for dim in range(3)]
        scalars.append(('<fluidscalar 0[0]>', component.𝒫))
    return scalars


def _gather_domains(component, values):
    """float64 (domains, len(values)) in domain order"""
    if component.comm is not None and component.nprocs > 1:
        return component.comm.all_gather_floats(list(values)).numpy()
    return np.asarray(values, dtype=np.float64).reshape(1, -1)


def _measure_ctx(component):
    # (the kernels use a context for its stream, launch checks and scratch memory only)
    if component.representation == 'particles':
        return component._store.mesh._ctx
    return component._mesh()._ctx


def _device_sums(ctx, device, x, n, stride, offset, ncols, start=None, count=None, nregions=0):
    out = torch.empty(SUMS_PER_COLUMN*ncols, dtype=torch.float64, device=device)
    check(raw().cg_measure_sums(ctx, _ptr(x), int(n), int(stride), int(offset), int(ncols),
                                _ptr(start), _ptr(count), int(nregions), _ptr(out)))
    return out.tolist()


def _grid_sums(component, grid, scale=1.0):
    """combine_sums over all domains of one fluid grid"""
    local = _device_sums(_measure_ctx(component), component.device, grid, grid.numel(), 1, 0, 1)
    return combine_sums(_gather_domains(component, local), component.gridsize**3, scale)


def _particle_momentum_sums(component, regions):
    """the 18 numbers of cg_measure_sums for the three columns of this domain's mom, read once"""
    if regions is not None:
        regions.finish_exchange()
        mom = regions.mom[regions.cur]
        ctx = regions.mesh._ctx
        if regions.count is None:
            return _device_sums(ctx, mom.device, mom, regions.n_dense, 3, 0, 3)
        return _device_sums(ctx, mom.device, mom, 0, 3, 0, 3, regions.start, regions.count,
                            regions.start.numel() - 1)
    mom = component.mom.contiguous()
    return _device_sums(_measure_ctx(component), component.device, mom, mom.shape[0], 3, 0, 3)


def measure(component, quantity, a=1.0, regions=None):
    """measure(component, quantity) of the reference (analysis.py:3860-4230) at scale factor a;
    collective over the x-slab domains.  regions: a particle component's particles in streaming
    form (distributed.RegionParticles).

      'v_max', 'v_rms'   particles: stepper.measure.  Fluids: fluid.v_max, and the rms bulk
                         velocity plus the global sound speed (0 without a J variable)
      'momentum'         (Σmom, σmom), two arrays of 3: of the particles' momenta, or of Vcell*J
      'ϱ'                (ϱ_bar, σϱ, ϱ_min) of a fluid
      'mass'             a**(-3*w_eff)*N*mass, or a**(-3*w_eff)*Vcell*Σϱ
      'discontinuity'    (names, Δdiff_max_list, Δdiff_max_normalized_list) over the fluid's
                         scalars: per dimension the largest |forward − backward difference|, and
                         that over the largest |difference| (0 where the former is 0)
    The sums are taken in double-double on the GPU and finished in decimal (combine_sums): the
    number of domains changes a sum by less than count·2⁻¹⁰⁰ Σ|x| and the extremes not at all."""
    from . import fluid, stepper
    name = component.name
    particles = component.representation == 'particles'
    if quantity in ('v_max', 'v_rms') and particles:
        return stepper.measure(component, quantity, a, regions)
    if quantity not in ('v_max', 'v_rms', 'momentum', 'ϱ', 'mass', 'discontinuity'):
        raise ConceptGPUError(f'measure(): quantity "{quantity}" not implemented')
    w_eff = component.w_eff(a=a)
    if particles:
        if quantity == 'momentum':
            parts = _gather_domains(component, _particle_momentum_sums(component, regions))
            sums = [combine_sums(parts[:, SUMS_PER_COLUMN*dim:SUMS_PER_COLUMN*(dim + 1)],
                                 component.N) for dim in range(3)]
            return np.array([s_.sum for s_ in sums]), np.array([s_.sigma for s_ in sums])
        if quantity == 'mass':
            return a**(-3*w_eff)*component.N*component.mass
        if quantity == 'ϱ':
            raise ConceptGPUError(f'The measure function was called with {name} and '
                                  "quantity='ϱ', but particle components do not have ϱ")
        raise ConceptGPUError(f'The measure function was called with {name} and '
                              "quantity='discontinuity', which is not applicable to particle "
                              'components')
    p = component.params
    N_elements = component.gridsize**3
    Vcell = p.boxsize**3/N_elements
    closure_class = component.boltzmann_closure == 'class'
    if quantity == 'v_max':
        return fluid.v_max(component, a, closure_class=closure_class)
    if quantity == 'v_rms':
        if component.boltzmann_order == 0 and not closure_class:
            return 0.0   # without J as a fluid variable no velocity exists
        if component.boltzmann_order == 0:
            raise ConceptGPUError(
                f'{name}: measure(): quantity "v_rms" with J as a linear fluid variable '
                '(boltzmann_order = 0, Boltzmann closure "class") is not implemented')
        fluid._check_scope(component, a, closure_class)
        out = torch.empty(SUMS_PER_COLUMN, dtype=torch.float64, device=component.device)
        check(raw().cg_measure_fluid_velocity(
            _measure_ctx(component), _ptr(component.ϱ), _ptr(component.𝒫),
            fluid._ptrs(list(component.J)), component.ϱ.numel(), float(p.light_speed**(-2)),
            _ptr(out)))
        # sqrt(Σ/N_elements): the mean of the squares, as the deviation of values about 0
        sums = combine_sums(_gather_domains(component, out.tolist()), N_elements)
        with decimal.localcontext() as ctx:
            ctx.prec = 2*17
            rms = float((decimal.Decimal(sums.sum)/N_elements).sqrt()) if sums.sum >= 0 \
                else math.nan
        return a**(3*w_eff - 2)*rms + p.light_speed*math.sqrt(component.w(a=a))/a
    if quantity == 'momentum':
        sums = [_grid_sums(component, J_dim, Vcell) for J_dim in component.J]
        return np.array([s_.sum for s_ in sums]), np.array([s_.sigma for s_ in sums])
    if quantity == 'ϱ':
        sums = _grid_sums(component, component.ϱ)
        return sums.mean, sums.sigma, sums.min
    if quantity == 'mass':
        return a**(-3*w_eff)*Vcell*_grid_sums(component, component.ϱ).sum
    # 'discontinuity'
    scalars = fluidscalar_names(component)
    names, Δdiff_max_list, Δdiff_max_normalized_list = [], [], []
    inv_h = 1/(p.boxsize/component.gridsize)
    out = torch.empty(6, dtype=torch.float64, device=component.device)
    for scalar_name, grid in scalars:
        lo, hi = fluid._neighbour_layers(component, [grid], 1)
        check(raw().cg_measure_discontinuity(
            _measure_ctx(component), _ptr(grid), fluid._halo_ptr(lo), fluid._halo_ptr(hi),
            component.gridsize, component.nxl, inv_h, _ptr(out)))
        maxima = _gather_domains(component, out.tolist()).max(axis=0)
        Δdiff_max, diff_max = maxima[:3], maxima[3:]
        names.append(scalar_name)
        Δdiff_max_list.append(Δdiff_max)
        Δdiff_max_normalized_list.append(np.array(
            [Δdiff_max[dim]/diff_max[dim] if Δdiff_max[dim] > 0 else 0 for dim in range(3)],
            dtype=np.float64))
    return names, Δdiff_max_list, Δdiff_max_normalized_list
