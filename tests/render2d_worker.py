"""Worker of tests/test_gpu_render2d.py: one rank of a P-rank x-slab 2D render.  The ranks share
cuda:0 and talk over gloo (test only; production is one GPU per rank over RCCL).  Every rank
projects its own layers — its own columns of the image for the axes y and z, a partial image
for axis x — and the images are summed in rank order, so every rank holds the render, which
must agree with the reference's (and so with one domain) and be the same on all ranks bit for
bit.  Arguments: names of goldens, or synthetic:N for the projections of a seeded mesh of size N
against a direct host sum (check_synthetic_on_domains of the test module)."""
import os
import sys
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
    from concept_amd import comm
    comm.init()
    c = comm.active()
    import test_gpu_render2d as t
    for name in sys.argv[1:]:
        if name.startswith('synthetic:'):
            # a seeded global array, every rank its own layers, against a direct host sum
            t.check_synthetic_on_domains(int(name.split(':')[1]), c)
            print(f'rank {rank}: {name} ok', flush=True)
            continue
        g = t.golden(name)
        comps = t.golden_components(g)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            images = t.check_against_golden(g, comps, tag=f'rank {rank} {name} ')
        for image in images:
            rows = c.all_gather_rows(torch.from_numpy(image).reshape(1, -1).cuda())
            assert all(torch.equal(rows[r], rows[0]) for r in range(world)), \
                'the ranks hold different images'
        print(f'rank {rank}: {name} ok', flush=True)
    dist.barrier()
    print(f'RANK{rank}-OK', flush=True)


if __name__ == '__main__':
    main()
