"""Worker of tests/test_gpu_powerspec.py: one rank of a P-rank x-slab power spectrum.  The
ranks share cuda:0 and talk over gloo (test only; production is one GPU per rank over RCCL).
Every rank bins its own Fourier rows; the partial bins are summed in rank order, so every
rank holds the spectrum, which must agree with the reference's (and so with one domain)."""
import os
import sys
import tempfile
import warnings

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from concept_amd import analysis, comm
    comm.init()
    import test_gpu_powerspec as t
    with tempfile.TemporaryDirectory() as tmp:
        for name in sys.argv[1:]:
            g = t.golden(name)
            comps = t.golden_components(g)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                decls = analysis.powerspec(comps, os.path.join(tmp, name), a=float(g['a']))
            t.check_against_golden(g, decls)
            print(f'rank {rank}: {name} ok', flush=True)
    dist.barrier()
    print(f'RANK{rank}-OK', flush=True)


if __name__ == '__main__':
    main()
