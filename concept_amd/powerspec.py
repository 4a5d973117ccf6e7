"""python -m concept_amd.powerspec SNAPSHOT [--params FILE] [--output-dir DIR]

The reference's `-u powerspec SNAPSHOT` utility (utilities.py:465-497): the power spectra that
powerspec_select / powerspec_options of the parameter file ask for, of the components of a
GADGET snapshot, at the scale factor of its header, written to
<output dir>/<output_bases['powerspec']>_<snapshot basename> (the output directory defaults to
the snapshot's own directory).  The box size is the snapshot's."""
import argparse
import os
import sys


def snapshot_utility(argv, prog, description, kind):
    """The part the snapshot utilities share (utilities.py:465-497): parse the command line,
    load the parameters with the snapshot's box size and the snapshot itself; returns
    (components, a, t, <output dir>/<output_bases[kind]>_<snapshot basename>)."""
    parser = argparse.ArgumentParser(prog=prog, description=description)
    parser.add_argument('snapshot')
    parser.add_argument('--params', default=None, help='parameter file')
    parser.add_argument('--output-dir', default=None)
    args = parser.parse_args(argv)
    import torch  # noqa: F401  (before the library, see concept_amd.lib)
    from . import commons, snapshot
    from .integration import Cosmology
    p = commons.load_params(args.params)
    head = snapshot.load(args.snapshot, only_params=True, params=p,
                         units=p.gadget_snapshot_params['units'])
    p = commons.load_params(args.params, boxsize=head.params['boxsize'])
    snap = snapshot.load(args.snapshot, params=p, units=p.gadget_snapshot_params['units'])
    components = snap.to_components()
    a = float(snap.params['a']) if p.enable_Hubble else 1.0
    t = None
    if p.enable_Hubble:
        cosmo = Cosmology(p)
        cosmo.init_time()
        t = cosmo.cosmic_time(a)
    output_dir = args.output_dir or os.path.dirname(os.path.abspath(args.snapshot))
    base = p.output_bases.get(kind, kind)
    # the snapshot's basename without its extension (utilities.py:465-497); the digits after
    # the point of a dump name such as snapshot_a=0.12 are no extension
    root, ext = os.path.splitext(os.path.basename(args.snapshot.rstrip('/')))
    name = root if ext and not ext[1:].isdigit() else root + ext
    filename = os.path.join(output_dir, f'{base}_{name}' if base else name)
    return components, a, t, filename


def main(argv=None):
    components, a, t, filename = snapshot_utility(
        argv, 'python -m concept_amd.powerspec', __doc__.split('\n\n')[1], 'powerspec')
    from . import analysis
    analysis.powerspec(components, filename, a=a, t=t)
    print(f'power spectrum written to "{filename}"')
    return filename


if __name__ == '__main__':
    main(sys.argv[1:])
