"""python -m concept_amd.render2D SNAPSHOT [--params FILE] [--output-dir DIR]

The reference's `-u render2D SNAPSHOT` utility (utilities.py:465-497): the 2D renders that
render2D_select / render2D_options of the parameter file ask for, of the components of a
GADGET snapshot, at the scale factor of its header, written to
<output dir>/<output_bases['render2D']>_<snapshot basename> plus the extensions of the data
file and the image (the output directory defaults to the snapshot's own directory); the
terminal image goes to stdout.  The box size is the snapshot's."""
import sys

from .powerspec import snapshot_utility


def main(argv=None):
    components, a, t, filename = snapshot_utility(
        argv, 'python -m concept_amd.render2D', __doc__.split('\n\n')[1], 'render2D')
    from . import render
    _, files = render.render2D(components, filename, a=a, t=t)
    for fn in files:
        print(f'2D render written to "{fn}"')
    return files


if __name__ == '__main__':
    main(sys.argv[1:])
