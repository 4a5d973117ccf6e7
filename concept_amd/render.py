"""concept_amd.render — 2D renders of the components (the reference's graphics.py:1027-1955).

  render2D()                     graphics.py:1027-1057
  get_render2D_declarations()    graphics.py:1168-1249 over analysis.get_output_declarations
                                 (graphics.py:1080-1143)
  compute_render2D()             graphics.py:1278-1336: interpolate_upstream(..., 'ρ', ...,
                                 output_space='Fourier') (interactions.interpolate_upstream,
                                 the one gravity uses) on mesh contexts of the roles
                                 'render2D' and 'render2D upstream', resize_grid
                                 (mesh.py:808-933) for the terminal image, the inverse
                                 transforms, then the projection in HIP (cg_render2d_project,
                                 csrc/cg_render.hip)
  projection_planes()            the plane range and fractions of project_render2D,
                                 graphics.py:1385-1400, 1482-1490
  enhance_render2D()             graphics.py:1568-1717: the binary search on the exponent on
                                 the host, its histograms, minima and maxima and the
                                 transformation of the pixels on the device
                                 (cg_render2d_minmax / _histogram / _apply)
  rescale_render2D()             graphics.py:1733-1755
  save_render2D_data()           graphics.py:1773-1815 (HDF5 with h5py, else .npz)
  save_render2D_image()          graphics.py:1832-1856
  augment_filename()             graphics.py:1859-1885
  display_terminal_render()      graphics.py:1901-1931 with set_terminal_colormap
                                 (graphics.py:1934-1954)
The images stay on the device until they are written; per iteration of the search only the
histogram counts and two numbers cross to the host."""
import collections
import math
import os
import sys
import warnings

import numpy as np
import torch

from . import analysis, commons
from . import comm as _comm
from .analysis import _components_str, _mesh
from .interactions import interpolate_upstream

# what a declaration holds (graphics.py:1241-1249): the components, which outputs to make,
# the resolved options, and the projections (device tensors by output key)
_outputs = ('data', 'image', 'terminalimage')
_options = ('gridsize', 'terminal_resolution', 'interpolation', 'deconvolve', 'interlace', 'axis',
            'extent', 'colormap', 'enhance')
Render2DDeclaration = collections.namedtuple(
    'Render2DDeclaration',
    ('components',) + tuple(f'do_{key}' for key in _outputs) + _options + ('projections',),
    defaults=(None,)*(2 + len(_outputs) + len(_options)))

# escape sequences of the terminal image (commons.py:679-685)
esc = '\x1b'
esc_normal = f'{esc}[0m'
esc_background = f'{esc}[48;5;{{}}m'
esc_set_color = f'{esc}]4;{{}};rgb:{{}}/{{}}/{{}}{esc}\\'

# numerical parameters of the enhancement (graphics.py:1599-1606)
shifting_factor = 0.28
exponent_min = 1e-2
exponent_max = 1e+2
exponent_tol = 1e-3
n_bins_min = 25
n_bins_fac = 1e-2
color_truncation_factor_lower = 0.005
color_truncation_factor_upper = 0.0001

_warned = set()


def _warn_once(key, message):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(message)


def _nprocs():
    c = _comm.active()
    return c.world if c is not None else 1


def _master():
    c = _comm.active()
    return c is None or c.rank == 0


# -- declarations ------------------------------------------------------------------------------
def terminal_resolution_for(gridsize, terminal_width, nprocs):
    """The terminal resolution used when none is set (graphics.py:1190-1201): the grid size
    capped at the terminal width, rounded down to a multiple of the number of processes (at
    least one per process), and doubled if that leaves it odd — the terminal image comes out of
    a slab-decomposed FFT and its rows are averaged in pairs."""
    resolution = min(int(gridsize), int(terminal_width))
    resolution -= resolution % nprocs
    resolution = resolution or nprocs
    return resolution if resolution % 2 == 0 else 2*resolution


def get_render2D_declarations(components):
    """graphics.py:1168-1231.  The projections are float64 tensors on the device; 'data' and
    'image' are one tensor, as they are one chunk of memory in the reference."""
    p = commons.params
    declarations = [
        Render2DDeclaration(components=combination, **specifications,
                            **{f'do_{key}': val for key, val in do.items()})
        for combination, do, specifications in analysis.get_output_declarations(
            'render2D', components, p.render2D_select, p.render2D_options)]
    device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device('cpu')
    for index, declaration in enumerate(declarations):
        terminal_resolution = declaration.terminal_resolution
        if terminal_resolution == -1:
            terminal_resolution = terminal_resolution_for(declaration.gridsize, p.terminal_width,
                                                          _nprocs())
        projections = {}
        for key in ('image', 'terminalimage', 'data'):
            if not getattr(declaration, f'do_{key}'):
                continue
            if key == 'data' and 'image' in projections:
                projections[key] = projections['image']
                continue
            gridsize = terminal_resolution if key == 'terminalimage' else declaration.gridsize
            projections[key] = torch.zeros((gridsize, gridsize), dtype=torch.float64,
                                           device=device)
        # (the reference's order of the keys: 'image', 'terminalimage', 'data')
        declarations[index] = declaration._replace(terminal_resolution=terminal_resolution,
                                                   projections=projections)
    return declarations


# -- the projection ----------------------------------------------------------------------------
def isint(x, abs_tol=1e-6):
    """commons.py:5239-5240"""
    return abs(x - round(x)) <= abs_tol


def projection_planes(gridsize, boxsize, extent):
    """The planes of project_render2D (graphics.py:1385-1400, 1468-1490) on one process:
    (plane_bgn, plane_end, frac_bgn, frac_end) — the planes [plane_bgn, plane_end) along the
    axis are summed, the first weighted by frac_bgn and the last by frac_end.  Where the
    reference finds no plane between the first and the last and an extent of at most one cell,
    the first plane alone is counted, with the extent in cells as its weight
    (graphics.py:1482-1490: frac_end is 0 then) — also for an extent that crosses into a second
    plane.  The reference does this on one process only: on several, where the two planes lie on
    different ranks, it adds frac_bgn and frac_end times the two planes.  Here the one-process
    result holds for any number of domains, so that a render does not depend on it."""
    cellsize = boxsize/gridsize
    float_index_global_bgn = extent[0]/cellsize
    float_index_global_end = extent[1]/cellsize
    if isint(float_index_global_bgn):
        float_index_global_bgn = round(float_index_global_bgn)
    if isint(float_index_global_end):
        float_index_global_end = round(float_index_global_end)
    plane_bgn = int(float_index_global_bgn)
    plane_end = int(math.ceil(float_index_global_end))
    frac_bgn = 1 - (float_index_global_bgn - plane_bgn)
    frac_end = 1 - (plane_end - float_index_global_end)
    start = plane_bgn + (frac_bgn > 0)
    stop = plane_end - (frac_end > 0)
    frac = float_index_global_end - float_index_global_bgn
    if 0 < frac_bgn and 0 < frac_end and 0 < frac <= 1 and start >= stop:
        frac_bgn = frac
        frac_end = 0
    return plane_bgn, plane_end, float(frac_bgn), float(frac_end)


def project_render2D(mesh, projection, axis, extent, a=1.0):
    """project_render2D (graphics.py:1374-1532) of the mesh's real-space values into the
    device tensor `projection`, in its final orientation and in units of mass.  Under
    comm.init() every domain projects its own layers and the domains' images are summed in
    rank order on every rank."""
    gridsize = mesh.gridsize
    cellsize = mesh.boxsize/gridsize
    plane_bgn, plane_end, frac_bgn, frac_end = projection_planes(gridsize, mesh.boxsize, extent)
    if plane_bgn == plane_end:  # no plane takes part (graphics.py:1437-1440)
        projection.zero_()
        return projection
    mesh.render2D_project(axis, plane_bgn, plane_end, frac_bgn, frac_end, (a*cellsize)**3,
                          out=projection)
    c = _comm.active()
    if c is not None and c.world > 1:
        projection.copy_(c.sum_in_rank_order(projection))
    return projection


def compute_render2D(declaration, a=1.0, timings=None):
    """graphics.py:1278-1336: fills declaration.projections (device tensors, on every rank).
    Of the terminal projection only the upper half of the rows holds data afterwards.
    timings: a dict that receives the seconds of the upstream interpolation (deposits and
    FFTs) and of the rest (inverse transforms and projections)."""
    components = declaration.components
    projections = declaration.projections
    termsize = declaration.terminal_resolution
    gridsizes_upstream = [analysis.upstream_gridsize(c, 'render2D') for c in components]
    if timings is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
    # quantity 'ρ' (mesh.py:1543-1549, 1713-1718)
    slab = interpolate_upstream(components, gridsizes_upstream, declaration.gridsize,
                                lambda c: a**(-3*(1 + c.w_eff(a=a))), declaration.interpolation,
                                declaration.deconvolve, declaration.interlace,
                                roles=('render2D', 'render2D upstream'))
    if timings is not None:
        ev[1].record()
    # the terminal image: a copy of the slab of terminal resolution, in real space
    # (resize_grid, mesh.py:808-933)
    grid_terminal = None
    if 'terminalimage' in projections:
        if termsize % 2 != 0:
            raise analysis.ConceptGPUError(
                f'Cannot produce terminal render with odd resolution {termsize}')
        grid_terminal = _mesh(termsize, 'render2D terminal')
        grid_terminal.copy_modes_from(slab, operation='=')
        grid_terminal.poisson_backward()
    slab.poisson_backward()
    for key, projection in projections.items():
        if key in ('data', 'image'):
            project_render2D(slab, projection, declaration.axis, declaration.extent, a)
            break
    projection = projections.get('terminalimage')
    if projection is not None:
        project_render2D(grid_terminal, projection, declaration.axis, declaration.extent, a)
        # a character cell is about twice as high as it is wide: consecutive pairs of rows are
        # averaged into the upper half of the rows (graphics.py:1330-1336)
        projection[:termsize//2] = 0.5*(projection[0::2] + projection[1::2])
    if timings is not None:
        ev[2].record()
        ev[2].synchronize()
        timings['upstream'] = ev[0].elapsed_time(ev[1])*1e-3
        timings['projection'] = ev[1].elapsed_time(ev[2])*1e-3
    return projections


# -- enhancement -------------------------------------------------------------------------------
def isclose(a, b, rel_tol=1e-9):
    """commons.py:5212-5227 with abs_tol = 0"""
    return abs(a - b) <= rel_tol*max(abs(a), abs(b))


def histogram_edges(first_edge, last_edge, n_bins):
    """the edges np.histogram(a, n_bins) uses for data between first_edge and last_edge"""
    if first_edge == last_edge:
        first_edge, last_edge = first_edge - 0.5, last_edge + 0.5
    return np.linspace(first_edge, last_edge, n_bins + 1, endpoint=True)


def search_exponent(histogram, size, n_bins, trace=None):
    """The binary search of enhance_render2D (graphics.py:1627-1681), branch for branch.
    histogram(exponent) returns the counts of np.histogram(projection**exponent, n_bins).
    trace: a list that receives (exponent, index_center) of every iteration."""
    exponent_lower = exponent_min
    exponent_upper = exponent_max
    exponent = 1
    index_min = -4
    index_max = -2
    target = int(n_bins*shifting_factor)
    while True:
        bins = histogram(exponent)
        # bins[0] is skipped: empty cells often leave a large spike there
        Σbins = size - int(bins[0])
        occupation = 0
        for index in range(1, n_bins):
            occupation += int(bins[index])
            if occupation >= Σbins//2:
                index_center = index
                break
        else:
            warnings.warn('Something went wrong during 2D render enhancement')
            exponent = 1
            break
        if trace is not None:
            trace.append((float(exponent), index_center))
        if index_center < target:
            exponent_upper = exponent
            index_min = index_center
        elif index_center > target:
            exponent_lower = exponent
            index_max = index_center
        else:
            break
        if index_max >= index_min and index_max - index_min <= 1:
            break
        if exponent/exponent_min < 1 + exponent_tol:
            exponent = exponent_min
            break
        elif exponent_max/exponent < 1 + exponent_tol:
            exponent = exponent_max
            break
        exponent = math.sqrt(exponent_lower*exponent_upper)
    return float(exponent)


def color_limits(bins, bin_edges, size, vmin, vmax):
    """The colour limits of enhance_render2D (graphics.py:1686-1711) from the histogram of the
    transformed pixels.  bins[0] is left out throughout.  vmin is the left edge of the bin
    below the first one at which the counts, summed upwards from bins[1], reach
    int(0.005*total); vmax is the right edge of the first bin at which the counts, summed
    downwards from the last bin, reach int(0.0001*total).  A limit whose fraction is never
    reached stays as passed."""
    counts = np.asarray(bins, dtype=np.int64)
    total = int(size) - int(counts[0])
    upwards = np.cumsum(counts[1:])
    reached = np.nonzero(upwards >= int(color_truncation_factor_lower*total))[0]
    if reached.size:
        vmin = bin_edges[reached[0]]            # bin reached[0] + 1: its left neighbour's edge
    downwards = np.cumsum(counts[:0:-1])
    reached = np.nonzero(downwards >= int(color_truncation_factor_upper*total))[0]
    if reached.size:
        vmax = bin_edges[len(counts) - reached[0]]  # bin len - 1 - reached[0]: its right edge
    return float(vmin), float(vmax)


def _minmax(mesh, image, exponent=1.0):
    vmin, vmax = mesh.render2D_minmax(image, exponent).tolist()
    return vmin, vmax


def _histogram(mesh, image, exponent, n_bins):
    edges = histogram_edges(*_minmax(mesh, image, exponent), n_bins)
    counts = mesh.render2D_histogram(image, exponent, commons.upload(edges, image.device))
    return counts.cpu().numpy(), edges


def rescale_image(mesh, image):
    """rescale_render2D (graphics.py:1733-1755) of one image (a contiguous device tensor), in
    place: the values in [0, 1], or ½ everywhere for a homogeneous, non-empty image"""
    vmin, vmax = _minmax(mesh, image)
    if vmin != 0 and vmax != 0 and isclose(vmin, vmax):
        mesh.render2D_apply(image, fill=0.5)
    else:
        with np.errstate(divide='ignore'):
            scale = float(np.float64(1)/np.float64(vmax - vmin))
        mesh.render2D_apply(image, shift=vmin, scale=scale)
    return image


def enhance_image(mesh, image, info=None):
    """enhance_render2D (graphics.py:1607-1717) of one image (a contiguous device tensor), in
    place: rescaled to [0, 1], raised to the exponent the search finds and truncated to the
    colour limits.  info: a dict that receives 'exponent', 'n_bins', 'vmin', 'vmax' and the
    search's 'trace'."""
    rescale_image(mesh, image)
    vmin, vmax = _minmax(mesh, image)
    if vmin == vmax:  # completely homogeneous projections cannot be enhanced
        return image
    size = image.numel()
    n_bins = max(int(n_bins_fac*size), n_bins_min)
    trace = []
    exponent = search_exponent(lambda e: _histogram(mesh, image, e, n_bins)[0], size, n_bins,
                               trace)
    mesh.render2D_apply(image, exponent=exponent)
    bins, bin_edges = _histogram(mesh, image, 1.0, n_bins)
    vmin, vmax = color_limits(bins, bin_edges, size, vmin, vmax)
    mesh.render2D_apply(image, vmin=vmin, vmax=vmax)
    if info is not None:
        info.update(exponent=exponent, n_bins=n_bins, vmin=vmin, vmax=vmax, trace=trace)
    return image


def _images(declaration):
    """(key, mesh whose stream the image kernels run on, contiguous device view) of the
    projections that are images; of the terminal image the upper half of the rows"""
    out = []
    for key, projection in declaration.projections.items():
        if key == 'data':
            continue
        if key == 'terminalimage':
            mesh = _mesh(declaration.terminal_resolution, 'render2D terminal')
            projection = projection[:projection.shape[0]//2]
        else:
            mesh = _mesh(declaration.gridsize, 'render2D')
        out.append((key, mesh, projection))
    return out


def enhance_render2D(declaration, info=None):
    """graphics.py:1568-1717; info: a dict that receives enhance_image's info per key"""
    if not declaration.enhance:
        return
    for key, mesh, image in _images(declaration):
        sub = {}
        enhance_image(mesh, image, sub)
        if info is not None:
            info[key] = sub


def rescale_render2D(declaration):
    """graphics.py:1733-1755"""
    for key, mesh, image in _images(declaration):
        rescale_image(mesh, image)


# -- files -------------------------------------------------------------------------------------
def augment_filename(filename, text, ext=''):
    """augment_filename (graphics.py:1859-1885): `text` goes into the file's name in front of
    its time stamp — '/out/render2D_a=0.5.png' with 'matter' becomes
    '/out/render2D_matter_a=0.5.png' — or at the end of the name if it carries no '_t=' or
    '_a='.  With both stamps present the text goes in front of the later one.  `ext` (with
    or without its point) is the extension the result ends on: it is taken off first if the
    name has it, anything else after a point is part of the name."""
    text = text.lstrip('_')
    ext = ext.lstrip('.')
    directory, name = os.path.split(filename)
    if ext and os.path.splitext(name)[1] == '.' + ext:
        name = name[:-len(ext) - 1]
    # where each stamp first shows up (0 if it does not); the later of the two takes the text
    first = {stamp: max(name.find(stamp), 0) for stamp in ('_t=', '_a=')}
    if first['_t='] == first['_a=']:
        name = f'{name}_{text}'
    else:
        stamp = max(first, key=first.get)
        cut = name.rfind(stamp)
        name = f'{name[:cut]}_{text}{name[cut:]}'
    if ext:
        name = f'{name}.{ext}'
    return os.path.join(directory, name)


def _dump_filename(declaration, filename, n_dumps, ext):
    for e in ('hdf5', 'png', 'npz'):
        filename = filename.removesuffix(f'.{e}')
    filename += ext
    if n_dumps > 1:
        filename = augment_filename(
            filename, '_'.join(c.name.replace(' ', '-') for c in declaration.components), ext)
    return filename


def save_render2D_data(declaration, filename, n_dumps, a=1.0, t=None):
    """graphics.py:1773-1815.  With h5py: <name>.hdf5 in the reference's layout (attributes
    and the dataset 'data').  Without: <name>.npz holding arrays of the same names.  Only
    rank 0 writes; returns the name of the file."""
    if not declaration.do_data or not _master():
        return None
    p = commons.params
    attrs = collections.OrderedDict()
    attrs['unit time'] = 'Gyr'
    attrs['unit length'] = 'Mpc'
    attrs['unit mass'] = '10¹⁰ m☉'
    attrs['boxsize'] = p.boxsize
    attrs['components'] = _components_str(declaration.components)
    attrs['axis'] = declaration.axis
    attrs['extent'] = tuple(declaration.extent)
    if p.enable_Hubble:
        attrs['a'] = float(a)
    attrs['t'] = float('nan') if t is None else float(t)
    data = declaration.projections['data'].cpu().numpy()
    try:
        import h5py
    except ImportError:
        h5py = None
    filename = _dump_filename(declaration, filename, n_dumps, '.hdf5' if h5py else '.npz')
    d = os.path.dirname(filename)
    if d:
        os.makedirs(d, exist_ok=True)
    if h5py is not None:
        with h5py.File(filename, mode='w') as hdf5_file:
            for key, val in attrs.items():
                hdf5_file.attrs[key] = val
            dset = hdf5_file.create_dataset('data', data.shape, dtype=np.float64)
            dset[...] = data
    else:
        _warn_once('h5py', 'h5py is not installed: 2D render data is written as .npz files '
                           '(the arrays carry the names of the HDF5 attributes and dataset)')
        np.savez(filename, data=data, **attrs)
    return filename


def save_render2D_image(declaration, filename, n_dumps):
    """graphics.py:1832-1856: the PNG through matplotlib's imsave.  Only rank 0 writes;
    returns the name of the file (None when nothing was written)."""
    if not declaration.do_image or not _master():
        return None
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        _warn_once('matplotlib', 'matplotlib is not installed: no 2D render images are written')
        return None
    filename = _dump_filename(declaration, filename, n_dumps, '.png')
    d = os.path.dirname(filename)
    if d:
        os.makedirs(d, exist_ok=True)
    plt.imsave(filename, declaration.projections['image'].cpu().numpy(),
               cmap=declaration.colormap, vmin=0, vmax=1)
    return filename


def terminal_colormap_sequence(colormap):
    """set_terminal_colormap (graphics.py:1934-1954): the 238 control sequences that remap
    the colour numbers 18-255 (a grey ramp without matplotlib)"""
    try:
        import matplotlib
        import matplotlib.cm
        import matplotlib.colors
        rgbs = getattr(matplotlib.cm, colormap)(np.linspace(0, 1, 238))[:, :3]
        hexes = [matplotlib.colors.rgb2hex(rgb) for rgb in rgbs]
    except ImportError:
        _warn_once('matplotlib terminal', 'matplotlib is not installed: the terminal image '
                                          'uses a grey colormap')
        hexes = ['#' + f'{int(round(255*v)):02x}'*3 for v in np.linspace(0, 1, 238)]
    return ''.join(esc_set_color.format(18 + i, *[h[c:c + 2] for c in range(1, 7, 2)])
                   for i, h in enumerate(hexes))


def terminal_ansi(image):
    """The ANSI image of display_terminal_render (graphics.py:1921-1929) of a host array of
    values in [0, 1]: per pixel a space on the background colour 18 + round(v*237)"""
    esc_space = f'{esc_background} '
    rows = []
    for row in np.asarray(image):
        rows.append(''.join(esc_space.format(18 + int(round(float(v)*237))) for v in row)
                    + f'{esc_normal}\n')
    return ''.join(rows)


def display_terminal_render(declaration, stream=None):
    """graphics.py:1901-1931: the colormap sequences, then the ANSI image of the upper half
    of the terminal projection's rows, written to `stream` (default: stdout) by rank 0"""
    if not declaration.do_terminalimage or not _master():
        return
    stream = sys.stdout if stream is None else stream
    projection = declaration.projections['terminalimage']
    image = projection[:projection.shape[0]//2].cpu().numpy()
    stream.write(terminal_colormap_sequence(declaration.colormap))
    stream.write(terminal_ansi(image))
    stream.flush()


def render2D(components, filename, a=1.0, t=None, stream=None, timings=None):
    """graphics.py:1027-1057: per declaration compute, save the data, enhance, rescale, save
    the image and display the terminal image.  a: the current scale factor (universals.a), t:
    the cosmic time.  Returns (declarations, names of the files written)."""
    declarations = get_render2D_declarations(components)
    n_dumps = sum(1 for d in declarations if d.do_data or d.do_image)
    files = []
    for declaration in declarations:
        compute_render2D(declaration, a, timings)
        files.append(save_render2D_data(declaration, filename, n_dumps, a, t))
        enhance_render2D(declaration)
        rescale_render2D(declaration)
        files.append(save_render2D_image(declaration, filename, n_dumps))
        display_terminal_render(declaration, stream)
    return declarations, [f for f in files if f]
