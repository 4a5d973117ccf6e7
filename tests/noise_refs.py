"""A plain restatement of csrc/cg_noise.hip, the primordial noise drawn on the device from numpy's
own streams, step for step as the kernel takes them: raw words of PCG64DXSM through the
jump-ahead table, the ziggurat of the standard exponential distribution classified in trips of T
words with the start flags from bit masks of 64 words (the kernel's ballots), the carry between
waves and trips, the prefix counts and the emitted values; then the phases and the slab.

Python integers for the 128-bit arithmetic, math.exp and math.log1p (the C library's, which
numpy's ziggurat calls) for the two rare functions, numpy for the rest.  The ziggurat tables are
read from the committed header concept_amd/csrc/cg_ziggurat_tables.h."""
import math
import os
import struct
import sys

import numpy as np

from concept_amd import ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'concept_amd', 'csrc', 'cg_ziggurat_tables.h')
sys.path.insert(0, os.path.join(REPO, 'tools'))
import numpy_ziggurat_tables  # noqa: E402

MASK64, MASK128 = 2**64 - 1, 2**128 - 1
ZIGGURAT_EXP_R = 7.69711747013104972
WAVE = 64


def tables():
    """ke (integers), we, fe (floats) of the committed header"""
    words = numpy_ziggurat_tables.read_header(HEADER)

    def as_double(w):
        return struct.unpack('<d', struct.pack('<Q', w))[0]
    return (words['ke_double'], [as_double(w) for w in words['we_double']],
            [as_double(w) for w in words['fe_double']])


def join128(row, at):
    return int(row[at]) | int(row[at + 1]) << 64


def dxsm(state):
    """pcg_cm_random_r's output for the state before its step"""
    hi, lo = state >> 64, (state & MASK64) | 1
    hi ^= hi >> 32
    hi = hi*ic.PCG_CHEAP_MULTIPLIER & MASK64
    hi ^= hi >> 48
    return hi*lo & MASK64


def jumped(state, inc, row):
    """the state `row` = (aᵏ, Sₖ) steps on"""
    return (join128(row, 0)*state + join128(row, 2)*inc) & MASK128


def to_double(w):
    return float(w >> 11)*(1.0/9007199254740992.0)


def start_flag(slow, lane, s_in):
    """k_noise_generate's start_flag: `slow` the mask of 64 words, lane 0..64"""
    below = MASK64 if lane >= 64 else (1 << lane) - 1
    fast_below = ~slow & below
    if fast_below:
        r = lane - 1 - (fast_below.bit_length() - 1)
    else:
        r = lane + (0 if s_in else 1)
    return not r & 1


def start_flags_plain(slow_flags, s_first):
    """s₀ = s_first, s_(p+1) = !(s_p && slow_p): what start_flag has to reproduce"""
    s, out = s_first, []
    for slow in slow_flags:
        out.append(s)
        s = not (s and slow)
    return out, s


def exponentials(state, inc, n, T, jump=None, stats=None):
    """the first n draws of random_standard_exponential of the stream (state, inc), the kernel's
    way: trips of T words (a multiple of 64).  stats, a dict, counts the carry cases met:
    'second word in next trip' (a slow draw whose second word is the next trip's first) and
    'slow run across trips' (the last word of a trip and the first of the next both slow)."""
    assert T % WAVE == 0
    ke, we, fe = tables()
    jump = ic.pcg64dxsm_jump_table(T) if jump is None else jump
    out = []
    carry, carry_word = False, 0
    while len(out) < n:
        words = [dxsm(jumped(state, inc, jump[p])) for p in range(T)]
        ri = [w >> 11 for w in words]
        idx = [(w >> 3) & 0xff for w in words]
        slow = [not r < ke[i] for r, i in zip(ri, idx)]
        masks = [sum(1 << l for l in range(WAVE) if slow[v*WAVE + l]) for v in range(T//WAVE)]
        # the waves in turn, then every lane of every wave
        s_in, starts = not carry, []
        for mask in masks:
            starts += [start_flag(mask, lane, s_in) for lane in range(WAVE)]
            s_in = start_flag(mask, WAVE, s_in)
        plain, s_next = start_flags_plain(slow, not carry)
        assert starts == plain and s_in == s_next
        emitted = []  # (lane, value): the prefix count of a lane is its place in this list
        for p in range(T):
            if starts[p]:
                if not slow[p]:
                    emitted.append((p, float(ri[p])*we[idx[p]]))
                continue
            first = words[p - 1] if p else carry_word
            ri1, idx1 = first >> 11, (first >> 3) & 0xff
            x = float(ri1)*we[idx1]
            U = to_double(words[p])
            if idx1 == 0:
                emitted.append((p, ZIGGURAT_EXP_R - math.log1p(-U)))
            elif (fe[idx1 - 1] - fe[idx1])*U + fe[idx1] < math.exp(-x):
                emitted.append((p, x))
        if stats is not None:
            if carry:
                stats['second word in next trip'] = stats.get('second word in next trip', 0) + 1
            if len(out) and slow[0] and stats.pop('_last slow', False):
                stats['slow run across trips'] = stats.get('slow run across trips', 0) + 1
            stats['_last slow'] = slow[-1]
        compact = [value for _, value in emitted]  # s_amp
        out += compact
        carry, carry_word = not s_in, words[-1]
        state = jumped(state, inc, jump[T])
    if stats is not None:
        stats.pop('_last slow', None)
    return np.array(out[:n], dtype=np.float64)


def uniforms(state, inc, n, T, jump=None):
    """the first n uniform doubles of the stream, word t by the jump-ahead table from the trip's
    first state"""
    jump = ic.pcg64dxsm_jump_table(T) if jump is None else jump
    out = []
    while len(out) < n:
        out += [to_double(dxsm(jumped(state, inc, jump[p]))) for p in range(T)]
        state = jumped(state, inc, jump[T])
    return np.array(out[:n], dtype=np.float64)


def slab(gridsize, fixed_amplitude=False, phase_shift=0, params=None, T=64):
    """generate_primordial_noise(gridsize, ...) of the 'distributed' scheme from the stream
    table, the order table and the store rule of cg_noise_generate: every stream drawn once"""
    g, nyquist = gridsize, gridsize//2
    streams = ic.noise_stream_table(g, fixed_amplitude, params)
    order = ic.noise_order_table(g)
    jump = ic.pcg64dxsm_jump_table(T)
    ki, kk = order[:, 0].astype(np.int64), order[:, 1].astype(np.int64)
    n = len(order)
    out = np.zeros((g, g, g + 2), dtype=np.float64)
    π = ic.π
    for row, κ in enumerate(range(-nyquist + 1, nyquist)):
        θ = -π + uniforms(join128(streams[row], 4), join128(streams[row], 6), n, T, jump)*(π - -π)
        if phase_shift:
            θ = θ + phase_shift
        if fixed_amplitude:
            r = 1.0
        else:
            E = exponentials(join128(streams[row], 0), join128(streams[row], 2), n, T, jump)
            r = np.sqrt(2.0*E)*(1/math.sqrt(2))
        re, im = r*np.cos(θ), r*np.sin(θ)
        own = (kk != 0) | (ki < 0) | ((ki == 0) & (κ < 0))
        out[κ % g, ki[own] % g, 2*kk[own]] = re[own]
        out[κ % g, ki[own] % g, 2*kk[own] + 1] = im[own]
        conj = (kk == 0) & ~((ki > 0) | ((ki == 0) & (κ > 0)))
        origin = conj & (ki == 0) & (κ == 0)
        re, im = np.where(origin, 0.0, re), np.where(origin, 0.0, im)
        out[-κ % g, -ki[conj] % g, 0] = re[conj]
        out[-κ % g, -ki[conj] % g, 1] = -im[conj]
    return out
