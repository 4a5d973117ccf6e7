"""Trajectory-level parity: whole runs of the time loop
against the reference's own main.timeloop() on the shapes of test/pure_python_pm/param and
test/pure_python_p3m/param (tests/golden/traj_*.npz: ~140 base steps from a_begin to a = 1,
matter + Λ background).

  * Timeloop.run(): the build computes everything itself — background, time-step integrals,
    base-step control (limiters, synchronisations at dumps and at changes of Δt), rungs.  Bars:
    every step's (t, a, Δt) within 1e-10 relative of the reference's; particle positions at every
    dump within the reference's own bar of test/pure_python_pm/analyze.py:125 (mean |Δx| / boxsize
    <= 1e-10) — asserted on the MAXIMUM over the particles.
  * stepper.timeloop (the streaming loop — kick + drift + tile sort in one pass — and the
    stepwise loop) replaying the reference's recorded integrals segment by segment.
All of it also on 2 and 4 x-slab domains (tests/test_gpu_distributed.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEY2 = 'a**(-3*w_eff₀-3*w_eff₁-1)'


def _component(g):
    from concept_amd import commons
    from concept_amd.species import Component
    p = commons.load_params(str(g['param_text']))
    c = Component('matter', 'matter', N=int(g['N']), mass=float(g['mass']))
    c.populate(g['pos_in'], 'pos')
    c.populate(g['mom_in'], 'mom')
    return p, c


def _pos_err(pos, ref, L):
    d = np.abs(pos - ref)
    return np.minimum(d, L - d).max()/L


@pytest.mark.parametrize('name', ['traj_pm_n8_g8', 'traj_p3m_n8_g24_r1', 'traj_p3m_n8_g24',
                                  'traj_pm_n8_g16', 'traj_p3m_n8_g32',
                                  # 16^3 particles, 60 % of them in three clumps, five rungs
                                  # populated, the shape of test/concept_vs_gadget_p3m/param
                                  'traj_p3m_n16_g32_clustered'])
def test_timeloop_run_vs_reference(golden, name, streaming=None):
    from concept_amd import stepper
    g = golden(name)
    p, c = _component(g)
    L = p.boxsize
    assert p.N_rungs == int(g['N_rungs'])
    dumps = []

    def on_dump(loop, dump_time):
        dumps.append((loop.cosmo.a, loop.cosmo.t, c.host('pos'), c.host('mom')))
    loop = stepper.Timeloop([c], on_dump=on_dump, streaming=streaming)
    loop.run()
    if str(g['method']) == 'pm' and streaming is not False:
        # the PM runs took the streaming form: one pass per long kick (+ one per drift that
        # could not ride with a kick), every guess about the drift after an init kick right
        n_kicks = int((g['kick_t'] >= 0).sum())
        assert n_kicks - 25 <= loop.stream_passes <= n_kicks + 25, (loop.stream_passes, n_kicks)
        assert loop.stream_wrong_guesses == 0
    else:
        assert loop.stream_passes == 0
    # the step sequence: number, cosmic time, scale factor and size of every base step
    hist = np.array(loop.history)
    assert hist.shape[0] == g['step_number'].shape[0], (hist.shape, g['step_number'].shape)
    assert np.array_equal(hist[:, 0], g['step_number'])
    for col, key in ((1, 'step_t'), (2, 'step_a'), (3, 'step_dt')):
        assert np.abs(hist[:, col]/g[key] - 1).max() <= 1e-10, key
    # the dumps
    assert len(dumps) == len(g['dump_a'])
    kick = np.abs(g['dump_mom'][-1] - g['mom_in']).max()
    for i, (a, t, pos, mom) in enumerate(dumps):
        assert a == g['dump_a'][i] and abs(t/g['dump_t'][i] - 1) <= 1e-12
        assert _pos_err(pos, g['dump_pos'][i], L) <= 1e-10, (i, a)
        assert np.abs(mom - g['dump_mom'][i]).max() <= 1e-9*kick, (i, a)
    assert dumps[-1][0] == g['dump_a'][-1]
    if g['dump_a'][-1] == 1.0:
        # the particles have really moved: several cells between the first and the last dump
        moved = np.abs(g['dump_pos'][-1] - g['pos_in'])
        assert np.minimum(moved, L - moved).max() > L/int(g['gridsize'])


@pytest.mark.parametrize('name', ['traj_pm_n8_g8', 'traj_pm_n8_g16'])
def test_timeloop_run_stepwise_vs_reference(golden, name):
    """the same runs with the separate kick and drift + sort passes (streaming = False)"""
    test_timeloop_run_vs_reference(golden, name, streaming=False)


@pytest.mark.parametrize('name', ['traj_pm_n8_g8', 'traj_p3m_n8_g24_r1', 'traj_pm_n8_g16'])
@pytest.mark.parametrize('streaming', [True, False])
def test_stepper_timeloop_replays_reference_integrals(golden, name, streaming):
    """stepper.timeloop with the integrals the reference recorded, call by call: a segment
    between two synchronisations is K½ D K D ... K; (with on_step = None the PM loop takes the
    streaming form, cg_gather_kick_drift_scatter; with a callback the separate passes)."""
    from concept_amd import stepper
    g = golden(name)
    p, c = _component(g)
    L = p.boxsize
    p3m = str(g['method']) == 'p3m'
    if p3m and streaming:
        pytest.skip('the streaming form is the PM loop')
    keys = [tuple(k.split('|')) if '|' in k else str(k) for k in g['integral_keys']]
    calls = [dict(zip(keys, v)) for v in g['integral_values']]
    cursor = [0]

    def pop(kind):
        cursor[0] += 1
        return calls[cursor[0] - 1]

    def pop_rungs(kind):
        d = pop(kind)
        return {(KEY2, 'matter', 'matter'): np.full(2, d[KEY2, 'matter', 'matter'])}
    # Segments between synchronisations, from who asked for each integral ('L0' / 'L1'
    # kick_long init / full, 'S' the init short kick, 'Dd' the drift and 'D' the rung kick of
    # driftkick_short): L0 [S] (Dd [D] L1)*n, then possibly a lone Dd — the last step before a
    # synchronisation time less than half a step away is a drift only, the kicks are there
    # already (main.py:1131-1135: t_start == t_end).
    ctx = [str(x) for x in g['integral_context']]
    group = ['Dd', 'D', 'L1'] if p3m else ['Dd', 'L1']
    head = ['L0', 'S'] if p3m else ['L0']
    segments = []
    i = 0
    while i < len(ctx):
        assert ctx[i:i + len(head)] == head, (i, ctx[i:i + 4])
        i += len(head)
        n = 0
        while ctx[i:i + len(group)] == group:
            n += 1
            i += len(group)
        tail = ctx[i:i + 1] == ['Dd']
        i += int(tail)
        segments.append((n, tail))
    replays = stepper.stream_replays
    dump_pos = list(g['dump_pos'])
    # the dumps happen at synchronisations, i.e. at ends of segments: the particle positions
    # at the end of a segment either equal the next dump's or belong to no dump
    n_dump = 0
    for n_steps, tail in segments:
        stepper.timeloop([c], n_steps, pop, pop_rungs if p3m else None,
                         on_step=None if streaming else (lambda step: None))
        if tail:
            stepper.drift([c], pop('full'))
        if n_dump < len(dump_pos) and _pos_err(c.host('pos'), dump_pos[n_dump], L) <= 1e-10:
            n_dump += 1
    assert cursor[0] == len(calls)
    assert n_dump == len(dump_pos)
    assert _pos_err(c.host('pos'), g['dump_pos'][-1], L) <= 1e-10
    kick = np.abs(g['dump_mom'][-1] - g['mom_in']).max()
    assert np.abs(c.host('mom') - g['dump_mom'][-1]).max() <= 1e-9*kick
    if streaming:
        assert stepper.stream_replays == replays   # (no region overflowed on the way)


def test_timeloop_wrong_guess_is_undone(golden):
    """The one speculative pass of the streaming loop: the drift after an init kick.  A
    limiter that drops between the choice of Δt at a synchronisation and the look at it after
    the init kick that follows (here: every limiter lowered by the on_step callback of the very
    first step, which runs between the two) synchronises half a step later (main.py:316-321),
    i.e. the drift taken with that kick was too long: the pass is undone and retaken.  The run
    must equal the stepwise one in its step sequence and, to rounding, in the particles."""
    from concept_amd import stepper
    g = golden('traj_pm_n8_g16')
    results = []
    for streaming in (None, False):
        p, c = _component(g)

        def on_step(loop):
            if loop.time_step == 0 and not getattr(loop, 'lowered', False):
                loop.lowered = True
                loop.fac_dynamical *= 0.3
                loop.fac_hubble *= 0.3
                loop.fac_pm *= 0.3
                loop.params.Δa_max_early *= 0.3
                loop.params.Δa_max_late *= 0.3
        loop = stepper.Timeloop([c], on_step=on_step, streaming=streaming)
        loop.run()
        results.append((np.array(loop.history), c.host('pos'), c.host('mom'),
                        loop.stream_wrong_guesses, loop.stream_passes))
    (h0, p0, m0, wrong, passes), (h1, p1, m1, _, none) = results
    assert passes > 0 and none == 0
    assert wrong >= 1, 'the scenario was meant to make a guess fail'
    assert h0.shape == h1.shape and np.abs(h0/np.where(h1 == 0, 1, h1) - 1)[:, 1:].max() <= 1e-12
    L = float(g['boxsize'])
    assert _pos_err(p0, p1, L) <= 1e-11
    assert np.abs(m0 - m1).max() <= 1e-10*np.abs(m1).max()


def test_streaming_timeloop_without_the_order_column(golden):
    """Component.keep_order = False: particles without identifiers whose memory order the loop
    may change (the reference's own contract) — no 64-bit column rides through the fused
    passes.  Same step sequence, and the same particles as a SET: the rows of (pos, mom),
    sorted, equal those of the ordered run."""
    from concept_amd import stepper
    g = golden('traj_pm_n8_g16')
    out = []
    for keep in (True, False):
        p, c = _component(g)
        c.keep_order = keep
        loop = stepper.Timeloop([c])
        loop.run()
        assert loop.stream_passes > 0
        rows = np.concatenate([c.host('pos', original_order=keep),
                               c.host('mom', original_order=keep)], 1)
        out.append((np.array(loop.history), rows[np.lexsort(rows.T[::-1])]))
    (h0, r0), (h1, r1) = out
    assert h0.shape == h1.shape and np.abs(h0/np.where(h1 == 0, 1, h1) - 1)[:, 1:].max() <= 1e-12
    L = float(g['boxsize'])
    assert r0.shape == r1.shape == (int(g['N']), 6)
    assert np.abs(r0[:, :3] - r1[:, :3]).max() <= 1e-11*L
    assert np.abs(r0[:, 3:] - r1[:, 3:]).max() <= 1e-10*np.abs(r1[:, 3:]).max()


def test_timeloop_overflow_of_the_speculative_pass(golden):
    """The speculative pass (kick + guessed drift after an init kick) overflows AND its guess
    turns out wrong: the replay on the exact path replaces the region objects, so the guess
    must not be undone from snapshots of the old ones (particles were corrupted and
    the kick applied twice).  The replay takes the kick only; the drift the loop then asks for
    is a pass of its own.  Must equal the stepwise run."""
    from concept_amd import stepper
    g = golden('traj_pm_n8_g16')
    results = []
    for streaming in (None, False):
        p, c = _component(g)

        def on_step(loop):
            if loop.time_step == 0 and not getattr(loop, 'lowered', False):
                loop.lowered = True
                loop.fac_dynamical *= 0.3
                loop.fac_hubble *= 0.3
                loop.fac_pm *= 0.3
                loop.params.Δa_max_early *= 0.3
                loop.params.Δa_max_late *= 0.3
                # the next pass is the init kick after the synchronisation this causes
                if loop.stream is not None:
                    stepper.force_replays = 1
        loop = stepper.Timeloop([c], on_step=on_step, streaming=streaming)
        replays = stepper.stream_replays
        loop.run()
        results.append((np.array(loop.history), c.host('pos'), c.host('mom'), c.host('ids'),
                        stepper.stream_replays - replays))
    assert stepper.force_replays == 0
    (h0, p0, m0, i0, r0), (h1, p1, m1, i1, _) = results
    assert r0 >= 1
    assert h0.shape == h1.shape and np.abs(h0/np.where(h1 == 0, 1, h1) - 1)[:, 1:].max() <= 1e-12
    L = float(g['boxsize'])
    o0, o1 = np.argsort(i0), np.argsort(i1)
    assert _pos_err(p0[o0], p1[o1], L) <= 1e-11
    assert np.abs(m0[o0] - m1[o1]).max() <= 1e-10*np.abs(m1).max()


def test_timeloop_streaming_at_north_star_size():
    """The time loop itself at the metric's size (2^28 particles / 1024^3 mesh, ΛCDM clock):
    a few base steps from a = 0.1 through stepper.Timeloop — background, integrals, limiters,
    v_rms measured on the regions, every long kick riding with its drift.  Properties: the
    streaming form was taken (one pass per kick), no guess failed, no region overflowed, every
    particle is still there, the clock arrived; prints the wall time per base step."""
    import time
    import torch
    from concept_amd import commons, stepper
    from concept_amd.species import Component
    n, N = 2**28, 1024
    p = commons.load_params({
        'boxsize': 1024.0, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.1,
        'output_times': {'a': (0.13,)},
        'potential_options': {'gridsize': {'gravity': {'pm': N}}},
        'select_forces': {'all': {'gravity': 'pm'}}})
    mass = p.ρ_mbar*p.boxsize**3/n
    c = Component('matter', 'matter', N=n, mass=mass)
    gen = torch.Generator(device='cuda').manual_seed(5)
    torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=gen, out=c.pos)
    c.pos.mul_(p.boxsize*(1 - 1e-13))
    # peculiar velocities of ~100 km/s: u = a ẋ -> mom = a m u
    u = 100*p.units.km/p.units.s
    torch.randn((n, 3), dtype=torch.float64, device='cuda', generator=gen, out=c.mom)
    c.mom.mul_(0.1*mass*u/3**0.5)
    ids_sum = n*(n - 1)//2
    steps = []
    def on_step(lp):
        torch.cuda.synchronize()
        steps.append(time.perf_counter())
    loop = stepper.Timeloop([c], on_step=on_step)
    replays = stepper.stream_replays
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    nsteps = loop.time_step
    assert nsteps >= 3 and loop.cosmo.a == pytest.approx(0.13, rel=1e-12)
    assert loop.stream_passes >= nsteps and loop.stream_wrong_guesses == 0
    assert stepper.stream_replays == replays
    assert c.N_local == n and int(c.ids.sum().item()) == ids_sum
    assert bool(((c.pos >= 0) & (c.pos < p.boxsize)).all())
    d = np.diff(np.array(steps))*1e3
    print('\nwall time between the beginnings of consecutive base steps (ms):',
          ' '.join(f'{v:.1f}' for v in d))
    print(f'Timeloop at 2^28 / 1024^3: {nsteps} base steps, {loop.stream_passes} passes in '
          f'{wall:.2f} s = {wall/max(loop.stream_passes, 1)*1e3:.1f} ms per pass (deposit + solve '
          f'+ fused kick/drift/sort + v_rms + host)')


def test_streaming_loop_through_structure_formation():
    """A whole run with real clustering — 64^3 particles on a 128^3 PM mesh from a displaced
    lattice at a = 0.05 to a = 1, ~120 base steps in which the tiles' populations change by
    factors — through the streaming form of the time loop and through the separate passes:
    same step sequence, every particle kept (identifiers a permutation), positions equal to
    what rounding allows after that many steps.  The streaming loop sizes its tile regions from
    the previous step's populations; where a region overflows it undoes and replays the pass
    (stepper.stream_replays is printed)."""
    from concept_amd import commons, stepper
    from concept_amd.species import Component
    n_side, gs, L = 64, 128, 64.0
    n = n_side**3
    rng = np.random.default_rng(2024)
    lat = (np.stack(np.meshgrid(*[np.arange(n_side)]*3, indexing='ij'), -1).reshape(-1, 3)
           + 0.5)*(L/n_side)
    # a smooth displacement field (a few long waves) + small-scale noise, growing mode
    k = 2*np.pi/L
    psi = np.zeros((n, 3))
    for d in range(3):
        for m in range(1, 4):
            ph = rng.uniform(0, 2*np.pi, 3)
            psi[:, d] += 0.35/m*np.sin(m*k*lat[:, (d + 1) % 3] + ph[0]) \
                * np.cos(m*k*lat[:, (d + 2) % 3] + ph[1])
    psi += rng.normal(0, 0.02, (n, 3))
    results = []
    for streaming in (None, False):
        p = commons.load_params({
            'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.05,
            'output_times': {'a': (1.0,)},
            'potential_options': {'gridsize': {'gravity': {'pm': gs}}},
            'select_forces': {'all': {'gravity': 'pm'}}})
        mass = p.ρ_mbar*L**3/n
        c = Component('matter', 'matter', N=n, mass=mass)
        loop = stepper.Timeloop([c], streaming=streaming)
        a0 = loop.cosmo.a
        pos = (lat + psi*a0/0.05) % L
        c.populate(pos, 'pos')
        c.populate(psi*mass*a0**2*loop.cosmo.hubble(a0), 'mom')
        replays = stepper.stream_replays
        loop.run()
        ids = c.host('ids', original_order=False)
        assert np.array_equal(np.sort(ids), np.arange(n))
        results.append((np.array(loop.history), c.host('pos'), loop.stream_passes,
                        stepper.stream_replays - replays))
    (h0, p0, passes, replays), (h1, p1, none, _) = results
    assert passes > 100 and none == 0
    assert h0.shape == h1.shape and h0.shape[0] > 100
    assert np.abs(h0[:, 1:]/h1[:, 1:] - 1).max() <= 1e-9
    d = np.abs(p0 - p1)
    d = np.minimum(d, L - d)
    # the two runs differ by rounding only (summation orders of v_rms and of the deposit); the
    # clustered end state amplifies that: mean over the particles, generous bar
    assert d.mean() <= 1e-7*L, d.mean()
    # it did cluster: the particles have left the lattice by several cells
    moved = np.abs(p1 - lat % L)
    assert np.minimum(moved, L - moved).max() > 4*L/gs
    print(f'\nstructure formation run: {h0.shape[0]} steps, {passes} streaming passes, '
          f'{replays} replayed, mean |dx| between the two forms {d.mean()/L:.2e} L, max '
          f'{d.max()/L:.2e} L')


def test_timeloop_writes_gadget_snapshots_at_the_dumps(golden, tmp_path):
    """The reference's run writes a snapshot at every dump time (main.dump): here
    Timeloop.snapshot_dumper → concept_amd.snapshot.save.  The files (double precision
    payloads) read back hold the reference's dump positions to its own bar and the momenta of
    the run; their names carry the dump's scale factor with the digits the reference's
    prepare_for_output would use."""
    import os
    from concept_amd import snapshot, stepper
    g = golden('traj_pm_n8_g8')
    p, c = _component(g)
    L = p.boxsize
    loop = stepper.Timeloop([c])
    loop.on_dump = loop.snapshot_dumper(str(tmp_path), dataformat={'POS': 64, 'VEL': 64})
    loop.run()
    files = loop.snapshots_written
    assert len(files) == len(g['dump_a'])
    # (a_begin = 0.02: two digits are needed for the initial time not to read 0.0)
    assert [os.path.basename(f) for f in files] == [f'snapshot_a={a:.2f}' for a in g['dump_a']]
    kick = np.abs(g['dump_mom'][-1] - g['mom_in']).max()
    for i, fn in enumerate(files):
        snap = snapshot.load(fn)
        # (the header's Time went through commons.correct_float, as in the reference's writer)
        assert snap.params['a'] == pytest.approx(g['dump_a'][i], rel=1e-14)
        assert snap.params['boxsize'] == pytest.approx(L, rel=1e-14)
        (comp,) = snap.components
        assert comp['name'] == 'GADGET halo' and comp['N'] == int(g['N'])
        assert comp['mass'] == pytest.approx(float(g['mass']), rel=1e-13)
        assert _pos_err(comp['pos'], g['dump_pos'][i], L) <= 1e-10
        assert np.abs(comp['mom'] - g['dump_mom'][i]).max() <= 1e-9*kick
    # and a run can start from one of them (snapshot.to_components)
    (restart,) = snapshot.load(files[0]).to_components()
    assert restart.N == int(g['N'])
    assert _pos_err(restart.host('pos'), g['dump_pos'][0], L) <= 1e-10


def test_p3m_timeloop_with_rungs_at_config3_size():
    """BASELINE configs[2]'s size through the time loop: 256^3 particles, P³M on a 512^3 mesh with
    the default short-range parameters and 8 rungs, a few base steps of the ΛCDM clock from
    a = 0.1 (kick_long, kick_short, driftkick_short with rung jumps; cg_shortrange_cells sweeps
    per active rung).  Properties: every particle is still there (identifiers a permutation),
    inside the box, momenta finite; the net momentum is a small fraction of what the forces
    exchanged; several rungs are populated and the
    base steps arrive on the dump time; prints the wall time per base step."""
    import time
    import torch
    from concept_amd import commons, stepper
    from concept_amd.species import Component
    n_side, N = 256, 512
    n = n_side**3
    p = commons.load_params({
        'boxsize': 512.0, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.1,
        'output_times': {'a': (0.11,)},
        'potential_options': {'gridsize': {'gravity': {'p3m': N}}},
        'select_forces': {'all': {'gravity': 'p3m'}}})
    assert p.N_rungs == 8
    mass = p.ρ_mbar*p.boxsize**3/n
    c = Component('matter', 'matter', N=n, mass=mass)
    gen = torch.Generator(device='cuda').manual_seed(11)
    torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=gen, out=c.pos)
    c.pos.mul_(p.boxsize*(1 - 1e-13))
    u = 30*p.units.km/p.units.s
    torch.randn((n, 3), dtype=torch.float64, device='cuda', generator=gen, out=c.mom)
    c.mom.mul_(0.1*mass*u/3**0.5)
    mom_in = c.mom.clone()   # (identifiers are the row numbers: ids[i] = i)
    steps, rungs_seen = [], set()

    def on_step(lp):
        torch.cuda.synchronize()
        steps.append(time.perf_counter())
        rungs_seen.update(int(r) for r in torch.unique(c.rung_indices).tolist())
    loop = stepper.Timeloop([c], on_step=on_step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert loop.time_step >= 3 and loop.cosmo.a == pytest.approx(0.11, rel=1e-12)
    assert c.N_local == n
    ids = torch.sort(c.ids).values
    assert bool((ids == torch.arange(n, device='cuda')).all())
    assert bool(((c.pos >= 0) & (c.pos < p.boxsize)).all()) and bool(torch.isfinite(c.mom).all())
    # the momentum the forces handed out, and what of it is left over in the sum: pairs on the
    # same rung exchange equal and opposite kicks; partners on different rungs are kicked with
    # their own rung's integrals (gravity.py:321-349), which agree only to the order of the
    # scheme — the total moves by a small fraction of what was exchanged, not by rounding
    dmom = c.mom[torch.argsort(c.ids)] - mom_in
    exchanged = float(dmom.abs().sum())
    drift = float(dmom.sum(0).abs().max())
    assert exchanged > 0 and drift <= 1e-3*exchanged, (drift, exchanged)
    assert len(rungs_seen) >= 2, rungs_seen   # close pairs of a random field sit on higher rungs
    d = np.diff(np.array(steps))
    print(f'\nP³M time loop at 256^3 / 512^3, 8 rungs: {loop.time_step} base steps in {wall:.2f} s; '
          f'between steps (s): ' + ' '.join(f'{v:.2f}' for v in d) + f'; rungs seen {sorted(rungs_seen)}; net momentum / exchanged = {drift/exchanged:.2e}')


def test_run_driven_by_a_parameter_file(golden, tmp_path):
    """The reference's way of running (param file: initial_conditions, output_dirs, output_times
    by kind, snapshot_type, gadget_snapshot_params): the initial snapshot is written from the
    trajectory golden's particles, a parameter file names it and asks for GADGET snapshots at two
    of the golden's dump times (and a power spectrum — a dump that writes nothing — at a third);
    get_initial_conditions() + Timeloop().run() then produce the reference run's particles in
    files of the requested format under the requested names."""
    import os
    from concept_amd import commons, snapshot, stepper
    g = golden('traj_pm_n8_g8')
    p0, c0 = _component(g)
    L = p0.boxsize
    ic = str(tmp_path/'ic')
    snapshot.save([{'name': 'GADGET halo', 'species': 'matter', 'N': int(g['N']),
                    'mass': float(g['mass']), 'pos': g['pos_in'], 'mom': g['mom_in'], 'ids': None}],
                  ic, a=p0.a_begin, dataformat={'POS': 64, 'VEL': 64})
    a_dumps = [float(a) for a in g['dump_a']]
    out = str(tmp_path/'out')
    text = str(g['param_text']) + f"""
initial_conditions = {ic!r}
output_dirs = {{'snapshot': {out!r}}}
output_bases = {{'snapshot': 'snap'}}
output_times = {{'snapshot': ({a_dumps[0]!r}, {a_dumps[-1]!r}), 'powerspec': {a_dumps[1]!r}}}
snapshot_type = 'gadget'
gadget_snapshot_params = {{'snapformat': 1, 'dataformat': {{'POS': 64, 'VEL': 64}}}}
"""
    p = commons.load_params(text)
    assert p.snapshot_times['a'] == (a_dumps[0], a_dumps[-1]) and len(p.output_times['a']) == 3
    comps = stepper.get_initial_conditions()
    assert [c.name for c in comps] == ['GADGET halo'] and comps[0].N == int(g['N'])
    loop = stepper.Timeloop(comps)
    loop.run()
    files = sorted(os.listdir(out))
    assert files == [f'snap_a={a_dumps[0]:.2f}', f'snap_a={a_dumps[-1]:.2f}'], files
    kick = np.abs(g['dump_mom'][-1] - g['mom_in']).max()
    for fn, i in zip(files, (0, len(a_dumps) - 1)):
        snap = snapshot.load(os.path.join(out, fn))
        assert snap.snapformat == 1
        (comp,) = snap.components
        # (the initial momenta went through a file: u = mom/(m a^1.5) and back, an ulp or two)
        assert _pos_err(comp['pos'], g['dump_pos'][i], L) <= 1e-10
        assert np.abs(comp['mom'] - g['dump_mom'][i]).max() <= 1e-9*kick


def test_timeloop_with_a_fluid_component(golden):
    """The hook that lets configs[4]'s shape RUN (VERDICT r3 missing 3): a fluid component
    rides through Timeloop — kicked by gravity() in every kick_long (its ϱ deposited, its J
    kicked), its own evolution left to the caller's fluid_drift(component, ᔑdt, a_end), called
    where main.py calls Component.drift() for fluids (drift_fluids, main.py:1279-1299: once per
    full base step, over the whole step).  With a uniform fluid (no force on the particles)
    and static time stepping (the same step sequence) the particles must arrive where they
    arrive without the fluid; without the hook the loop refuses the fluid."""
    import torch
    from concept_amd import commons, stepper
    from concept_amd.lib import ConceptGPUError
    from concept_amd.species import Component
    g = golden('traj_pm_n8_g16')

    def make(with_fluid):
        text = (str(g['param_text']) + '\nstatic_timestepping = lambda a: 0.02 + 0*a\n'
                + "select_forces = {'all': {'gravity': 'pm'}}\n")
        p = commons.load_params(text)
        c = Component('matter', 'matter', N=int(g['N']), mass=float(g['mass']))
        c.populate(g['pos_in'], 'pos')
        c.populate(g['mom_in'], 'mom')
        comps = [c]
        if with_fluid:
            gs = 16
            fl = Component('neutrinos', 'neutrino', gridsize=gs, boltzmann_order=1)
            fl.populate(np.full((gs, gs, gs), 1e-3*c.ϱ_bar), 'ϱ')
            fl.populate(np.zeros((gs, gs, gs)), '𝒫')
            for d in range(3):
                fl.populate(np.zeros((gs, gs, gs)), 'J', d)
            comps.append(fl)
        return p, comps

    p, comps = make(True)
    with pytest.raises(ConceptGPUError, match='fluid_drift'):
        stepper.Timeloop(comps)
    calls = []

    def fluid_drift(component, ᔑdt, a_end):
        assert component.name == 'neutrinos' and ᔑdt['1'] > 0
        assert ('a**(-3*w_eff)', 'neutrinos') in ᔑdt
        calls.append((a_end, ᔑdt['1']))
    loop = stepper.Timeloop(comps, fluid_drift=fluid_drift)
    loop.run()
    n_full = len(loop.history)
    assert len(calls) >= n_full - 2 and len(calls) <= n_full + 2, (len(calls), n_full)
    assert all(b > a for (a, _), (b, _) in zip(calls, calls[1:]))   # in time order
    assert abs(calls[-1][0] - 1.0) <= 1e-9                            # the last step ends at a = 1
    # the time spanned by the fluid's drifts is the run's
    assert sum(dt for _, dt in calls) == pytest.approx(loop.cosmo.t - loop.history[0][1], rel=1e-9)
    J = comps[1].host('J')
    assert np.abs(J).max() > 0                      # the particles pulled on the fluid
    assert np.array_equal(comps[1].host('ϱ'), np.full((16, 16, 16), 1e-3*comps[0].ϱ_bar))
    pos_f, mom_f = comps[0].host('pos'), comps[0].host('mom')
    p, comps0 = make(False)
    loop0 = stepper.Timeloop(comps0, streaming=False)
    loop0.run()
    assert len(loop0.history) == len(loop.history)
    L = float(g['boxsize'])
    assert _pos_err(pos_f, comps0[0].host('pos'), L) <= 1e-9
    kick = np.abs(comps0[0].host('mom') - g['mom_in']).max()
    assert np.abs(mom_f - comps0[0].host('mom')).max() <= 1e-8*kick


def test_timeloop_with_a_fluid_component_dumps_snapshots(golden, tmp_path):
    """a fluid riding along (fluid_drift) and snapshot times together — the GADGET
    writer holds particle components only, the dumper leaves the fluid out (with a warning, once)
    instead of failing at the first dump."""
    from concept_amd import commons, snapshot, stepper
    from concept_amd.species import Component
    g = golden('traj_pm_n8_g16')
    text = (str(g['param_text']) + '\nstatic_timestepping = lambda a: 0.05 + 0*a\n'
            + "select_forces = {'all': {'gravity': 'pm'}}\n")
    commons.load_params(text)
    c = Component('matter', 'matter', N=int(g['N']), mass=float(g['mass']))
    c.populate(g['pos_in'], 'pos')
    c.populate(g['mom_in'], 'mom')
    gs = 16
    fl = Component('neutrinos', 'neutrino', gridsize=gs, boltzmann_order=1)
    fl.populate(np.full((gs, gs, gs), 1e-3*c.ϱ_bar), 'ϱ')
    loop = stepper.Timeloop([c, fl], fluid_drift=lambda comp, ᔑdt, a_end: None)
    loop.on_dump = loop.snapshot_dumper(str(tmp_path), 'snap')
    with pytest.warns(UserWarning, match='particle components only'):
        loop.run()
    assert len(loop.snapshots_written) == len(g['dump_a']) >= 1
    (comp,) = snapshot.load(loop.snapshots_written[-1]).components
    assert comp['N'] == int(g['N'])


def test_p3m_timeloop_with_dense_tiles_equals_the_cells_sweep(monkeypatch):
    """A clustered box (80 % of 64^3 particles in 8 Gaussian blobs: tiles of several hundred
    particles) through the P³M time loop with 8 rungs, twice: with the dense tiles' sweep
    (cg_shortrange_dense.hip, the default from 64 particles per tile on) and with the half-tile
    cells everywhere (CONCEPT_GPU_SR_DENSE_MIN=0).  The two differ in the order of the additions
    only: same steps, same rungs, positions equal to 1e-9 of the box after the run."""
    import torch
    from concept_amd import commons, stepper
    from concept_amd.species import Component
    n, N, L = 64**3, 128, 128.0

    def run(dense):
        if dense == '0':
            monkeypatch.setenv('CONCEPT_GPU_SR_DENSE_MIN', '0')
        else:
            monkeypatch.delenv('CONCEPT_GPU_SR_DENSE_MIN', raising=False)
        p = commons.load_params({
            'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.1,
            'output_times': {'a': (0.105,)},
            'potential_options': {'gridsize': {'gravity': {'p3m': N}}},
            'select_forces': {'all': {'gravity': 'p3m'}}})
        mass = p.ρ_mbar*L**3/n
        c = Component('matter', 'matter', N=n, mass=mass)
        gen = torch.Generator(device='cuda').manual_seed(21)
        pos = torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=gen)*L
        centres = torch.rand((8, 3), dtype=torch.float64, device='cuda', generator=gen)*L
        which = torch.randint(0, 8, (n,), device='cuda', generator=gen)
        blob = centres[which] + torch.randn((n, 3), dtype=torch.float64, device='cuda',
                                            generator=gen)*(L/40)
        keep = torch.rand(n, dtype=torch.float64, device='cuda', generator=gen) < 0.2
        c.pos.copy_(torch.where(keep[:, None], pos, torch.remainder(blob, L)).clamp_(0, L*(1 - 1e-13)))
        c.mom.zero_()
        loop = stepper.Timeloop([c])
        loop.run()
        order = torch.argsort(c.ids)
        return loop.time_step, c.pos[order].clone(), c.rung_indices[order].clone()

    steps0, pos0, rungs0 = run('0')
    steps1, pos1, rungs1 = run('1')
    assert steps0 == steps1 and steps0 >= 2
    d = (pos1 - pos0).abs()
    d = torch.minimum(d, L - d)
    assert float(d.max()) <= 1e-9*L, float(d.max())
    assert float((rungs0 != rungs1).double().mean()) <= 1e-4   # (a particle on a rung's border)
    assert int(rungs0.max()) >= 2


def test_rung_loop_in_two_passes_equals_the_separate_calls(monkeypatch):
    """The rung loop's production form (a sub-step as two passes over the particles, the first
    inside the cell list's counting pass, populations counted before the jumps are applied, the
    sweeps by active receiver / by active-first blocks) against the reference's call sequence
    (drift, flag_rung_jumps, nullify_Δ, sweep with rung gathers, apply_Δmom,
    convert_Δmom_to_acc, apply_rung_jumps, set_rungs_N: main.py:1347-1624) on a clustered box of
    48^3 particles with several rungs populated, base step by base step."""
    import torch
    from concept_amd import commons, stepper
    from concept_amd.mesh import PotentialMesh
    from concept_amd.species import Component
    n_side, N = 48, 96
    n = n_side**3

    def run(fuse):
        monkeypatch.setattr(stepper.RungStepper, 'fuse_substeps', fuse)
        # (the separate calls with the plain lists of the reference's loop)
        monkeypatch.setattr(PotentialMesh, 'SHORTRANGE_BY_CELL_MAX', 0.16 if fuse else -1.0)
        p = commons.load_params({
            'boxsize': float(N), 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
            'output_times': {'a': (0.5,)},
            'potential_options': {'gridsize': {'gravity': {'p3m': N}}},
            'select_forces': {'all': {'gravity': 'p3m'}}})
        c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*p.boxsize**3/n)
        g = torch.Generator(device='cuda').manual_seed(4)
        pos = torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=g)*N
        blob = N/2 + torch.randn((n, 3), dtype=torch.float64, device='cuda', generator=g)*(N/30)
        pick = torch.rand(n, device='cuda', generator=g) < 0.5
        pos = torch.where(pick[:, None], torch.remainder(blob, N), pos).clamp_(0, N*(1 - 1e-13))
        c.populate(pos.cpu().numpy(), 'pos')
        c.populate(np.zeros((n, 3)), 'mom')
        snaps = []

        class Enough(Exception):
            pass

        def on_step(lp):
            snaps.append((lp.cosmo.t, lp.Δt, list(c.rungs_N), c.host('pos'), c.host('mom')))
            if len(snaps) > 6:
                raise Enough
        loop = stepper.Timeloop([c], on_step=on_step)
        try:
            loop.run()
        except Enough:
            pass
        return snaps
    a, b = run(False), run(True)
    assert len(a) == len(b) == 7
    assert max(len([v for v in s[2] if v]) for s in a) >= 3      # several rungs populated
    kick = np.abs(a[-1][4]).max()
    for i, (x, y) in enumerate(zip(a, b)):
        # the same clock (the base step follows v_rms: sums of momenta that agree to rounding)
        assert abs(x[0]/y[0] - 1) <= 1e-12 and abs(x[1]/y[1] - 1) <= 1e-10, i
        d = np.abs(x[3] - y[3])
        assert np.minimum(d, N - d).max() <= 1e-10*N, i
        assert np.abs(x[4] - y[4]).max() <= 1e-9*kick, i
        # (a rung assignment can differ where an acceleration sits on a rung's edge to rounding)
        assert sum(abs(u - v) for u, v in zip(x[2], y[2])) <= 2e-4*n, (i, x[2], y[2])
