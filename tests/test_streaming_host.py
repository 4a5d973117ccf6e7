"""Host logic of the streaming form of the PM time loop (no GPU): what one pass
calls and in which order, the replay of a pass that overflowed, the speculative pass of
Timeloop.kick_long with a right and a wrong guess, lending the particles to a dump, the hand-back
at the end and on unwinding.  Components, their regions and the mesh are recording stubs; the
whole sequence of calls is compared with literal lists, and every factor with the expression
written out here in the order of the code, bit for bit.  A region's snapshot() returns a new
token per call, so that a restore from a stale snapshot shows up in the list.

Every case but test_undo_is_refused_once_the_regions_are_replaced (an operation the earlier
form did not have) passed on the form of the loop before StreamingPM, with begin() below written
for that form's names and, in the lists of the cases through Timeloop.kick_long, the second set
of snapshots that kick_long then took of its own before its pass."""
import types

import pytest

BOX, GRID = 100.0, 32
DECONV, C, LONG_RANGE, E = 4, -1.25e3, False, 0.0
MASS = {'A': 1.7, 'B': 0.43}
ORDER = {'A': 2, 'B': 4}
KICK_KEY = ('a**(-3*w_eff)', 'component')
OVERFLOW, NOT_IN_TILE, STALE = 'CG_ERR_BUCKET_OVERFLOW', 'CG_ERR_NOT_IN_TILE', \
    'CG_ERR_STALE_HISTOGRAM'


def begin(env, loop=None):
    """Start streaming: stepper.timeloop and Timeloop find env's plan (or None) through
    interactions.pm_streaming_plan; a Timeloop made by env.loop() gets its not-streaming state
    and then decides for itself.  The one place that knows how the loop keeps that state."""
    from concept_amd import interactions
    plan = None if env.no_plan else interactions.StreamingPlan(
        mesh=env.mesh, gridsize=GRID, deconv_order=DECONV, C=C, long_range=LONG_RANGE, E=E,
        force='gravity', method='pm')
    env.monkeypatch.setattr(interactions, 'pm_streaming_plan', lambda components: plan)
    if loop is not None:
        loop.stream = loop._guess = None
        loop._begin_streaming()


def integrals(t0, t1):
    """time-step integrals that tell their interval (and the components) apart"""
    Δ = t1 - t0
    return {'interval': (t0, t1), '1': Δ, 'a**(-2)': 1.3*Δ,
            ('a**(-3*w_eff)', 'A'): 0.9*Δ, ('a**(-3*w_eff)', 'B'): 0.8*Δ,
            ('a**(-3*w_eff-1)', 'A'): 0.7*Δ, ('a**(-3*w_eff-1)', 'B'): 0.6*Δ}


INIT, FULL = integrals(0.0, 0.5), integrals(0.0, 1.0)


class Component(types.SimpleNamespace):
    """(a namespace that can be a dictionary's key, as Timeloop._v_rms uses it)"""
    __hash__, __eq__ = object.__hash__, object.__eq__


class Regions:
    def __init__(self, env, name):
        self.env, self.name, self.snapshots = env, name, 0

    def deposit(self, contribution, accumulate=False):
        self.env.log.append(('deposit', self.name, contribution, accumulate))

    def kick_drift_sort(self, diff_order, kick_factor, dt_over_mass):
        self.env.log.append(('kick_drift_sort', self.name, diff_order, kick_factor, dt_over_mass))

    def finish_exchange(self):
        self.env.log.append(('finish_exchange', self.name))

    def snapshot(self):
        self.env.log.append(('snapshot', self.name))
        self.snapshots += 1
        return ('snap', self.name, self.snapshots - 1)

    def restore(self, snap):
        self.env.log.append(('restore', self.name, snap))


class Env:
    """the stubs of one case and the log they write"""

    def __init__(self, monkeypatch, comm=False):
        from concept_amd import interactions, lib, stepper
        self.monkeypatch, self.stepper, self.lib = monkeypatch, stepper, lib
        self.log, self.flags, self.any, self.shortrange, self.no_plan = [], [], [], [], False
        env, log = self, self.log
        self.params = types.SimpleNamespace(boxsize=BOX)

        class Mesh:
            name, comm = 'mesh', None

            def fold_ghosts_start(self):
                log.append(('fold_ghosts_start',))
                return 'fold'

            def poisson_solve(self, deconv_order, C, long_range, E, fold_finish=None, fill=False):
                log.append(('poisson_solve', deconv_order, C, long_range, E, fold_finish, fill))

            def zero(self):
                log.append(('zero',))

            def error_flags(self):
                log.append(('error_flags',))
                return env.flags.pop(0) if env.flags else 0
        self.mesh = Mesh()
        if comm:
            self.mesh.comm = types.SimpleNamespace(any=self._any)

        def kick_particles(mesh, receiver, force, method, ᔑdt, ᔑdt_key):
            log.append(('kick_particles', mesh.name, receiver.name, force, method,
                        ᔑdt['interval'], ᔑdt_key))

        def measure(component, quantity, a, regions=None):
            log.append(('measure', component.name, quantity, a, regions and regions.name))
            return 2.0
        monkeypatch.setattr(interactions, '_kick_particles', kick_particles)
        monkeypatch.setattr(interactions, 'find_interactions',
                            lambda components, kind: list(self.shortrange))
        monkeypatch.setattr(stepper, 'measure', measure)
        monkeypatch.setattr(stepper, 'force_replays', 0)
        monkeypatch.setattr(stepper, 'stream_replays', 0)

    def _any(self, flag):
        self.log.append(('any', flag))
        return self.any.pop(0) if self.any else flag

    def queue(self, *flags):
        """what mesh.error_flags() answers, call by call (0 once the queue is empty)"""
        self.flags += [getattr(self.lib, f) if isinstance(f, str) else f for f in flags]

    def component(self, name, hand_back_raises=None):
        log, taken = self.log, []

        def to_regions(mesh):
            log.append(('to_regions', name, mesh.name))
            taken.append(Regions(self, f'{name}{len(taken)}'))
            return taken[-1]

        def from_regions(rp, collective=True):
            log.append(('from_regions', name, rp.name, collective))
            if hand_back_raises is not None:
                raise hand_back_raises

        def drift_sort(ᔑdt, a=1.0, mesh=None):
            log.append(('drift_sort', name, ᔑdt['interval'], mesh.name))
        return Component(
            name=name, mass=MASS[name], params=self.params, representation='particles',
            forces={'gravity': 'pm'}, use_rungs=False,
            potential_differentiations={'gravity': {'pm': ORDER[name]}},
            to_regions=to_regions, from_regions=from_regions, drift_sort=drift_sort)

    def components(self, names='AB', **kw):
        return [self.component(name, **kw) for name in names]

    def loop(self, names='AB', streaming=None, on_dump=None):
        """a Timeloop as far as its streaming methods look at it, at t = 0"""
        loop = object.__new__(self.stepper.Timeloop)
        loop.cosmo = types.SimpleNamespace(t=0.0, a=0.5)
        loop.components = loop.particles = self.components(names)
        loop.integrals = integrals
        loop.Δt_reltol = 1e-9
        loop.streaming, loop.on_dump = streaming, on_dump
        loop._next_drift = None
        loop.stream_passes = loop.stream_wrong_guesses = 0
        return loop

    def take(self):
        out = list(self.log)
        self.log.clear()
        return out


@pytest.fixture
def env(monkeypatch):
    return Env(monkeypatch)


# -- the expected calls, every factor written out -------------------------------------------
def contribution(name, ᔑdt):
    """interactions._particle_contribution (mesh.py:1550-1573), in its order"""
    x = ᔑdt['a**(-3*w_eff-1)', name]/ᔑdt['1']
    x *= MASS[name]
    x *= float(GRID)**(-3)*(GRID/BOX)**3
    return x


def taken(names='AB'):
    return [('to_regions', name, 'mesh') for name in names]


def handed_back(regions, collective=True):
    return [('from_regions', r[0], r, collective) for r in regions]


def a_pass(regions, kick=None, drift=None, zero=False, comm=None):
    """the calls of one pass over `regions` (names like 'A0': component A's first regions) up
    to the look at the error flags; comm: the local overflow flag mesh.comm.any is asked with"""
    out = []
    if kick is not None:
        out += [('deposit', r, contribution(r[0], kick), k > 0) for k, r in enumerate(regions)]
        out += [('fold_ghosts_start',),
                ('poisson_solve', DECONV, C, LONG_RANGE, E, 'fold', True)]
    elif zero:
        out += [('zero',)]
    out += [('snapshot', r) for r in regions]
    for r in regions:
        factor = MASS[r[0]]*(-kick['a**(-3*w_eff)', r[0]]) if kick is not None else 0.0
        Δt_over_mass = drift['a**(-2)']/MASS[r[0]] if drift is not None else 0.0
        out += [('kick_drift_sort', r, ORDER[r[0]], factor, Δt_over_mass)]
    out += [('finish_exchange', r) for r in regions]
    out += [('error_flags',)]
    if comm is not None:
        out += [('any', comm)]
    return out


def a_replay(regions, snapshots, kick=None, drift=None):
    """the pass over `regions` undone from its own snapshots (their serial numbers) and taken
    on the exact path"""
    out = []
    for r, serial in zip(regions, snapshots):
        out += [('restore', r, ('snap', r, serial)), ('from_regions', r[0], r, True)]
        if kick is not None:
            out += [('kick_particles', 'mesh', r[0], 'gravity', 'pm', kick['interval'], KICK_KEY)]
        if drift is not None:
            out += [('drift_sort', r[0], drift['interval'], 'mesh')]
        out += [('to_regions', r[0], 'mesh')]
    return out


def run_timeloop(env, components, n_steps=2):
    begin(env)
    env.stepper.timeloop(components, n_steps, {'init': INIT, 'full': FULL}.__getitem__)
    return env.take()


# -- 1-5: stepper.timeloop -------------------------------------------------------------------
def test_timeloop_takes_n_steps_plus_one_passes(env):
    """K½ D K D K: accumulate False then True, one fold and one solve per pass, no drift with
    the last kick (0.0 exactly), then one collective hand-back per component"""
    R = ['A0', 'B0']
    log = run_timeloop(env, env.components())
    assert log == (taken() + a_pass(R, INIT, FULL) + a_pass(R, FULL, FULL) + a_pass(R, FULL)
                   + handed_back(R))
    assert [e[3] for e in log if e[0] == 'deposit'] == [False, True]*3
    assert [e[0] for e in log].count('fold_ghosts_start') == 3
    assert [e[0] for e in log].count('poisson_solve') == 3
    last = [e for e in log if e[0] == 'kick_drift_sort'][-2:]
    assert [repr(e[4]) for e in last] == ['0.0', '0.0']
    assert env.stepper.stream_replays == 0


@pytest.mark.parametrize('flag', [OVERFLOW, NOT_IN_TILE])
def test_overflow_replays_the_pass_from_its_own_snapshots(env, flag):
    """the middle pass overflows: restored from the snapshots THAT pass took (the second of
    each region), taken on the exact path, and the next pass runs on the new regions"""
    env.queue(0, flag)
    log = run_timeloop(env, env.components())
    R, R1 = ['A0', 'B0'], ['A1', 'B1']
    assert log == (taken() + a_pass(R, INIT, FULL)
                   + a_pass(R, FULL, FULL) + a_replay(R, [1, 1], FULL, FULL)
                   + a_pass(R1, FULL) + handed_back(R1))
    assert env.stepper.stream_replays == 1


def test_force_replays_counts_down(env):
    env.monkeypatch.setattr(env.stepper, 'force_replays', 1)
    log = run_timeloop(env, env.components('A'))
    assert log == (taken('A') + a_pass(['A0'], INIT, FULL) + a_replay(['A0'], [0], INIT, FULL)
                   + a_pass(['A1'], FULL, FULL) + a_pass(['A1'], FULL) + handed_back(['A1']))
    assert env.stepper.force_replays == 0 and env.stepper.stream_replays == 1


def test_another_domain_overflowed(monkeypatch):
    """local flags 0, but mesh.comm.any answers True for the second pass: a replay; without a
    comm, any() is never asked (test_timeloop_takes_n_steps_plus_one_passes: no 'any')"""
    env = Env(monkeypatch, comm=True)
    env.any += [False, True]
    log = run_timeloop(env, env.components('A'))
    assert log == (taken('A') + a_pass(['A0'], INIT, FULL, comm=False)
                   + a_pass(['A0'], FULL, FULL, comm=False) + a_replay(['A0'], [1], FULL, FULL)
                   + a_pass(['A1'], FULL, comm=False) + handed_back(['A1']))
    assert env.stepper.stream_replays == 1


def test_other_error_flags_raise_and_unwind(env):
    """a flag the loop cannot recover from: ConceptGPUError with the label; every component is
    handed back without the collective part, the second although the first one's hand-back
    raises, and the original exception is the one that arrives"""
    env.queue(0, STALE)
    components = [env.component('A', hand_back_raises=RuntimeError('hand-back')),
                  env.component('B')]
    begin(env)
    with pytest.raises(env.lib.ConceptGPUError) as err:
        env.stepper.timeloop(components, 2, {'init': INIT, 'full': FULL}.__getitem__)
    assert str(err.value) == (f'streaming time loop: device error flags '
                              f'{env.lib.CG_ERR_STALE_HISTOGRAM:#x} in step 1')
    R = ['A0', 'B0']
    assert env.take() == (taken() + a_pass(R, INIT, FULL) + a_pass(R, FULL, FULL)
                          + handed_back(R, collective=False))


def test_overflow_next_to_another_flag_raises(env):
    env.queue(env.lib.CG_ERR_BUCKET_OVERFLOW | env.lib.CG_ERR_STALE_HISTOGRAM)
    begin(env)
    with pytest.raises(env.lib.ConceptGPUError, match='in step 0'):
        env.stepper.timeloop(env.components('A'), 1, {'init': INIT, 'full': FULL}.__getitem__)
    assert env.take() == (taken('A') + a_pass(['A0'], INIT, FULL)
                          + handed_back(['A0'], collective=False))
    assert env.stepper.stream_replays == 0


# -- 6-11: Timeloop.kick_long / driftkick_short ----------------------------------------------
ထ = float('inf')
KICK = integrals(0.0, 0.5)   # the init kick of Δt = 1 at t = 0


def streaming_loop(env, **kw):
    loop = env.loop(**kw)
    begin(env, loop)
    assert env.take() == taken(kw.get('names', 'AB'))
    return loop


def test_right_guess_is_one_pass(env):
    loop = streaming_loop(env)
    loop._next_drift = (0.0, 1.0)
    loop.kick_long(1.0, ထ, 'init')
    loop.driftkick_short(1.0, ထ)
    assert env.take() == a_pass(['A0', 'B0'], KICK, integrals(0.0, 1.0))
    assert (loop.stream_passes, loop.stream_wrong_guesses) == (1, 0)


def test_wrong_guess_is_undone_and_retaken(env):
    """restore with the tokens of the speculative pass, the same kick alone (no drift: 0.0),
    then the drift the loop asks for alone (no deposit, no solve, no zero; factor 0.0)"""
    loop = streaming_loop(env)
    R = ['A0', 'B0']
    loop._next_drift = (0.0, 1.0)
    loop.kick_long(1.0, ထ, 'init')
    assert env.take() == a_pass(R, KICK, integrals(0.0, 1.0))
    loop.driftkick_short(0.5, ထ)
    log = env.take()
    assert log == ([('restore', r, ('snap', r, 0)) for r in R]
                   + a_pass(R, KICK) + a_pass(R, None, integrals(0.0, 0.5)))
    sorts = [e for e in log if e[0] == 'kick_drift_sort']
    assert [repr(e[4]) for e in sorts[:2]] == ['0.0', '0.0']
    assert [repr(e[3]) for e in sorts[2:]] == ['0.0', '0.0']
    assert (loop.stream_passes, loop.stream_wrong_guesses) == (1, 1)
    assert env.stepper.stream_replays == 0


def test_wrong_guess_with_no_drift_to_take(env):
    """the loop asks for no drift at all (t_start == t_end): the kick-only retake, no more"""
    loop = streaming_loop(env, names='A')
    loop._next_drift = (0.0, 1.0)
    loop.kick_long(1.0, ထ, 'init')
    env.take()
    loop.driftkick_short(1.0, 0.0)
    assert env.take() == [('restore', 'A0', ('snap', 'A0', 0))] + a_pass(['A0'], KICK)
    assert (loop.stream_passes, loop.stream_wrong_guesses) == (1, 1)


def test_no_drift_predicted(env):
    loop = streaming_loop(env, names='A')
    loop.kick_long(1.0, ထ, 'init')
    assert env.take() == a_pass(['A0'], KICK)
    loop.driftkick_short(1.0, ထ)
    assert env.take() == a_pass(['A0'], None, integrals(0.0, 1.0))
    assert (loop.stream_passes, loop.stream_wrong_guesses) == (1, 0)


def test_kick_of_no_length_takes_no_pass(env):
    loop = streaming_loop(env, names='A')
    loop.kick_long(1.0, 0.0, 'full')
    assert env.take() == [] and loop.stream_passes == 0


def test_drift_before_any_kick_zeroes_the_mesh_once(env):
    loop = streaming_loop(env, names='A')
    loop.driftkick_short(1.0, ထ)
    assert env.take() == a_pass(['A0'], None, integrals(0.0, 1.0), zero=True)
    loop.driftkick_short(0.5, ထ)
    assert env.take() == a_pass(['A0'], None, integrals(0.0, 0.5))
    assert loop.stream_passes == 0


def test_replayed_speculative_pass_leaves_nothing_outstanding(env):
    """kick_long's pass overflows: the replay takes the kick only (no drift_sort), and the
    drift the loop asks for next — although it is the predicted one — is a pass of its own, on
    the new regions, with nothing restored"""
    loop = streaming_loop(env)
    env.queue(OVERFLOW)
    loop._next_drift = (0.0, 1.0)
    loop.kick_long(1.0, ထ, 'init')
    R, R1 = ['A0', 'B0'], ['A1', 'B1']
    assert env.take() == a_pass(R, KICK, integrals(0.0, 1.0)) + a_replay(R, [0, 0], KICK)
    loop.driftkick_short(1.0, ထ)
    assert env.take() == a_pass(R1, None, integrals(0.0, 1.0))
    assert (loop.stream_passes, loop.stream_wrong_guesses) == (1, 0)
    assert env.stepper.stream_replays == 1


# -- 12-14: dumps, v_rms, run() ----------------------------------------------------------------
def test_dump_lends_the_particles(env):
    """hand-back, the callback, regions taken again on the plan's mesh; the next pass uses
    them and restores nothing"""
    loop = streaming_loop(env, on_dump=lambda loop, dump_time: env.log.append(
        ('on_dump', dump_time)))
    loop.kick_long(1.0, ထ, 'init')
    env.take()
    loop._dump('now')
    assert env.take() == handed_back(['A0', 'B0']) + [('on_dump', 'now')] + taken()
    loop.driftkick_short(1.0, ထ)
    assert env.take() == a_pass(['A1', 'B1'], None, integrals(0.0, 1.0))
    loop.on_dump = None
    loop._dump('now')
    assert env.take() == []


def test_undo_is_refused_once_the_regions_are_replaced(env):
    """after a lend and after a replay the last pass's snapshots describe buffers that no
    longer exist: undo() refuses, and restores nothing"""
    loop = streaming_loop(env, names='A')
    stream = loop.stream
    stream.kick_drift(KICK, FULL)
    with stream.lend():
        pass
    env.take()
    with pytest.raises(env.lib.ConceptGPUError, match='undo'):
        stream.undo()
    env.queue(OVERFLOW)
    stream.kick_drift(KICK, FULL)
    env.take()
    with pytest.raises(env.lib.ConceptGPUError, match='undo'):
        stream.undo()
    assert env.take() == []
    # a pass that was not replayed can be undone, once
    stream.kick_drift(KICK, FULL)
    env.take()
    stream.undo()
    assert env.take() == [('restore', 'A2', ('snap', 'A2', 0))]
    with pytest.raises(env.lib.ConceptGPUError, match='undo'):
        stream.undo()


def test_v_rms_measures_on_the_regions_of_that_component(env):
    loop = streaming_loop(env)
    A, B = loop.components
    state = {'a': 0.5, 'v_rms': {}}
    assert loop._v_rms(B, state) == 2.0 and loop._v_rms(A, state) == 2.0
    assert loop._v_rms(B, state) == 2.0     # (measured once per state)
    assert env.take() == [('measure', 'B', 'v_rms', 0.5, 'B0'),
                          ('measure', 'A', 'v_rms', 0.5, 'A0')]
    loop = env.loop(streaming=False)
    begin(env, loop)
    loop._v_rms(loop.components[0], {'a': 0.25, 'v_rms': {}})
    assert env.take() == [('measure', 'A', 'v_rms', 0.25, None)]


def test_run_hands_back_at_the_end_and_on_unwinding(env):
    """an exception out of _run: hand-back without the collective part, a second exception
    from the hand-back swallowed, the first one arrives; a normal end hands back collectively"""
    boom = KeyboardInterrupt('boom')

    def fail():
        raise boom
    loop = env.loop()
    loop.components[1].from_regions = env.component(
        'B', hand_back_raises=RuntimeError('hand-back')).from_regions
    begin(env, loop)
    loop._run = fail
    with pytest.raises(KeyboardInterrupt) as err:
        loop.run()
    assert err.value is boom
    assert env.take() == taken() + handed_back(['A0', 'B0'], collective=False)
    loop = streaming_loop(env)
    loop._run = lambda: None
    loop.run()
    assert env.take() == handed_back(['A0', 'B0'])
    loop._v_rms(loop.components[0], {'a': 0.5, 'v_rms': {}})   # no longer streaming
    assert env.take() == [('measure', 'A', 'v_rms', 0.5, None)]


# -- 15: not streaming -------------------------------------------------------------------------
def not_streaming(env, loop):
    loop._v_rms(loop.components[0], {'a': 0.5, 'v_rms': {}})
    loop._run = lambda: None
    loop.run()
    return env.take() == [('measure', 'A', 'v_rms', 0.5, None)]


def test_streaming_false_never_streams(env):
    loop = env.loop(streaming=False)
    begin(env, loop)
    assert not_streaming(env, loop)


def test_a_short_range_interaction_never_streams(env):
    env.shortrange.append(('gravity', 'p3m', [], []))
    for streaming in (None, True):
        loop = env.loop(streaming=streaming)
        begin(env, loop)
        assert not_streaming(env, loop)


def test_no_plan(env):
    env.no_plan = True
    loop = env.loop()
    begin(env, loop)
    assert not_streaming(env, loop)
    loop = env.loop(streaming=True)
    with pytest.raises(env.lib.ConceptGPUError) as err:
        begin(env, loop)
    assert str(err.value) == ('Timeloop(streaming=True): not the default PM configuration '
                              '(interactions.pm_streaming_plan)')
    assert not_streaming(env, loop)
