"""bench.py keeps its contract under every flag it documents: one JSON line on stdout with the
driver's keys; with --full also `roofline` and (unless switched off) `cpu_baseline`.  A plain run
carries the headline figures only and --dump-outputs writes what its last step left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
        'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline'}


def run(*flags, env=None):
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--workload', 'tiny',
                        '--steps', '2', '--warmup', '1', '--full'] + list(flags),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # exactly one line on stdout
    d = json.loads(lines[0])
    assert KEYS <= set(d), KEYS - set(d)
    assert d['steps'] == 2 and d['warmup'] == 1 and d['value'] > 0 and d['dtype'] == 'f64'
    r = d['roofline']
    assert {'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'} <= set(r)
    assert 0 < r['frac'] <= 1
    for k in d.get('kernels', {}).values():
        assert k['frac_hbm'] <= 1
    return d


@pytest.mark.parametrize('flags', [
    (), ('--no-fused',), ('--no-sort',), ('--no-prepare',), ('--split-poisson',),
    ('--dist', 'lattice'), ('--dist', 'clustered'), ('--dist', 'zeldovich', '--seed', '2'),
    ('--thermal', '0'), ('--p3m',),
    ('--p3m', '--dist', 'clustered')])
def test_bench_flags(flags):
    d = run('--no-cpu-baseline', *flags)
    assert d['n_gpus'] == 1 and 'workload' in d['config']


def test_bench_cpu_baseline_and_sharded_paths():
    d = run()  # with the CPU baseline leg
    cb = d['cpu_baseline']
    assert cb['kind'] == 'port' and cb['value'] > 0 and cb['cores'] >= 1 and cb['sample']
    # the N > 1 code path with one rank (RCCL), and two self-spawned ranks sharing the GPU (gloo)
    d = run('--no-cpu-baseline', env={'CONCEPT_BENCH_FORCE_DIST': '1'})
    assert d['n_gpus'] == 1 and 'stages_ms_rank0' in d
    d = run('--no-cpu-baseline', '--gpus', '2')
    assert d['n_gpus'] == 2 and d['transport']['bound'] == 'xgmi'
    lm = d['link_model']   # the prediction beside the measured stages
    assert lm['predicted_step_ms'] > 0 and lm['transpose_ms_at_link_rate'] > 0
    assert lm['measured_step_ms'] == pytest.approx(d['ms_per_step'], rel=1e-3)
    assert d['config']['particles'] == 32**3


def run_workload(workload, *flags, steps=2, warmup=1, timeout=1500):
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', str(steps),
                        '--warmup', str(warmup), '--no-cpu-baseline', '--full']
                       + (['--workload', workload] if workload else []) + list(flags),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                       env=dict(os.environ))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert KEYS <= set(d), KEYS - set(d)
    return d


def test_bench_eight_ranks_at_config2_size():
    """First contact of `bench.py --gpus 8` with a real workload: the
    ACTUAL command at BASELINE configs[1]'s size — 256^3 particles / 512^3 mesh on 8 x-slab
    domains, here as 8 self-spawned ranks sharing the one GPU over gloo — runs to its JSON
    line, keeps every particle, reports the stages and carries the link model.  And it is
    self-verifying: the box is a function of (seed, identifier), the 1-rank
    run of the same command leaves the id-keyed sample the 8-rank run compares its own with —
    positions to 1e-12 of the box, momenta to 1e-12 of their rms."""
    one = run_workload('c2_256c_512')
    v1 = one['verify']
    assert v1['ok'] and v1['particles'] == 256**3 and v1['timed_vs_replay_rel'] <= 1e-12
    assert os.path.exists(os.path.join(REPO, v1['written_to']))
    d = run_workload('c2_256c_512', '--gpus', '8')
    v = d['verify']
    assert v['ok'] is True, v
    assert v['reference'] == v1['written_to'] and v['sample'] == 512
    assert v['max_pos_err_over_boxsize'] <= 1e-12 and v['max_mom_err_over_rms'] <= 1e-12
    assert v['particles'] == 256**3 and v['sum_mom2_rel_err'] <= 1e-12
    assert d['ranks_seen']['world'] == 8 and \
        sorted(r for r, _ in d['ranks_seen']['rank_device']) == list(range(8))
    ppr = d['particles_per_rank']
    assert sum(ppr['counts']) == 256**3 and 1.0 <= ppr['max_over_mean'] < 1.01
    assert d['n_gpus'] == 8 and d['config']['particles'] == 256**3
    assert d['config']['parallelism'] == 'xslab8' and d['scaling'] == 'strong'
    lm = d['link_model']
    assert lm['predicted_step_ms'] > 0 and lm['bytes_per_peer_per_transpose'] == 512**3*8//64 \
        or lm['bytes_per_peer_per_transpose'] > 0
    assert lm['measured_step_ms'] == pytest.approx(d['ms_per_step'], rel=1e-3)
    assert {'exchange+deposit', 'poisson+transposes+halos', 'kick_drift_sort'} \
        <= set(d['stages_ms_rank0'])
    assert d['emigrants_per_step'] > 0   # (thermal momenta: particles really change domain)
    assert d['per_gpu']['particles'] == 256**3//8


def test_bench_config4_shape_on_one_gpu():
    """--workload c4_nonlinnu_*: BASELINE configs[4]'s shape (param/example_nonlinnu:36-45) through
    Component.drift_sort / gravity() / apply_Δmom on one GPU — three mesh solves per long kick,
    a phase with its moved bytes per interaction."""
    d = run_workload('c4_nonlinnu_tiny')
    assert d['interactions'] == ['p3m: matter <- matter', 'pm: matter <- neutrino',
                                 'pm: neutrino <- matter, neutrino']
    assert set(d['phases']) == {'drift_sort', 'short_range'} | {'long: ' + s for s in d['interactions']}
    assert all(v['ms'] > 0 and v['moved_GB'] > 0 for v in d['phases'].values())
    assert d['config']['particles'] == 32**3 and d['config']['fluid_gridsize'] == 16
    # fractions in the phase's own unit: the pair sweep against the FP64 issue rate (executed
    # tests counted on the device), the others against the HBM rate
    sr = d['phases']['short_range']
    assert 'frac_hbm' not in sr and sr['bound'] == 'valu_fp64' and 0 < sr['frac_valu_fp64'] <= 1
    assert sr['tests_per_hit'] >= 1 and 0 < sr['lane_use'] <= 1
    assert all(0 < v['frac_hbm'] <= 1 for k, v in d['phases'].items() if k != 'short_range')
    r = d['roofline']
    assert 0 < r['frac'] <= 1
    assert (r['unit'], r['bound']) in {('pair-tests/s', 'valu_fp64'), ('GB/s', 'hbm')}
    assert (r['kernel'] == 'short_range') == (r['bound'] == 'valu_fp64')


def test_bench_weak_and_dry_links():
    """--weak: the per-GPU work fixed (2^25 particles, ~1.3e8 cells per GPU); --dry-links: the
    transposes replaced by device sleeps at one xGMI link's rate, the pipelined schedule of the
    transposing solve exercised and its overlap with the transforms reported."""
    d = run_workload(None, '--weak')
    assert d['scaling'] == 'weak' and d['config']['particles'] == 2**25 \
        and d['config']['gridsize'] == 512
    d = run_workload(None, '--weak', '--gpus', '2')
    assert d['scaling'] == 'weak' and d['n_gpus'] == 2
    assert d['config']['particles'] == 2**26 and d['config']['gridsize'] == 640
    assert 'rocFFT' in d['per_gpu']['fft_backend']
    d = run_workload('c2_256c_512', '--gpus', '8', '--dry-links')
    dl = d['dry_links']
    assert dl['rate_GBps_per_link'] == pytest.approx(76.8)
    assert dl['links_ms_per_solve'] > 0 and dl['transforms_alone_ms'] > 0
    # 2 transposes of 512^3*8/64 B per peer at 76.8 GB/s
    assert dl['links_ms_per_solve'] == pytest.approx(2*512**3*8/64/76.8e9*1e3*(512 + 16)/512,
                                                    rel=0.15)
    # (with the ranks sharing one GPU the hand-offs between the streams of eight processes
    # cost more than the sleeps: the fraction is reported, not asserted)
    assert 'overlap_fraction' in dl and dl['solve_ms'] > 0


def test_bench_rung_loop_leg():
    """--rung-loop: the P3M time loop with 8 rungs (configs.c2_p3m_rungs of the default line) —
    base steps timed between their beginnings, the loop's calls grouped by HIP events."""
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--workload', 'tiny',
                        '--rung-loop', 'clustered', '--steps', '4'],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.strip()][-1])
    assert d['base_steps_timed'] == 4 and d['ms_per_base_step'] > 0 and d['particles_kept']
    assert d['sub_steps_per_base_step'] >= 1 and d['sweeps_per_base_step'] >= 0
    g = d['gpu_ms_per_base_step_by_call']
    assert {'drift_flag_nullify', 'apply_convert_jumps_populations', 'long_range_kick'} <= set(g)
    assert sum(d['rung_populations_at_the_end']) == 32**3
    assert d['gpu_ms_per_base_step_in_calls'] <= 1.05*d['ms_per_base_step_min_max'][1]


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) times --steps steps and prints the headline figures only; with
    --dump-outputs it writes the particles its last step left, float64, and two runs of the same
    command start from the same particles: their outputs agree to the last bits the order of
    the device atomics leaves open."""
    out = {}
    for tag in ('a', 'b'):
        p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1',
                            '--workload', 'tiny', '--steps', '3', '--warmup', '1',
                            '--dump-outputs', str(tmp_path/tag)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'} <= set(d)
        assert d['steps'] == 3 and d['warmup'] == 1 and d['value'] > 0 and d['ms_per_step'] > 0
        assert d['metric'] == 'PM particle-updates/sec' and d['unit'] == 'particle-updates/s'
        assert d['higher_is_better'] is True and d['dtype'] == 'f64'
        assert d['value'] == pytest.approx(32**3/(d['ms_per_step']*1e-3), rel=1e-9)
        assert not {'roofline', 'kernels', 'verify', 'configs', 'cpu_baseline'} & set(d)
        out[tag] = {k: np.load(tmp_path/tag/(k + '.npy')) for k in ('pos', 'mom', 'totals')}
        assert all(a.dtype == np.float64 for a in out[tag].values())
        assert sum(os.path.getsize(tmp_path/tag/f) for f in os.listdir(tmp_path/tag)) <= 64 << 20
    a, b = out['a'], out['b']
    assert a['pos'].shape == a['mom'].shape == (32**3, 3) and a['totals'][0] == 32**3
    L = 64.0
    assert np.all((a['pos'] >= 0) & (a['pos'] < L))
    assert np.abs(a['pos'] - b['pos']).max() <= 1e-12*L
    assert np.abs(a['mom'] - b['mom']).max() <= 1e-12*np.sqrt((a['mom']**2).mean())
    assert np.allclose(a['totals'], b['totals'], rtol=1e-12)
