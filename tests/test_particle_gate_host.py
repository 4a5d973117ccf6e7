"""The gate of the particle entries (cg_internal.h, next to cgk_substep_flush), read from the
sources: every extern "C" entry that takes live particle arrays begins with one gate line, and no
entry flushes a deferred sub-step pass or voids the prepared drift histogram by a line of its own."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    'concept_amd', 'csrc')
# pos*, mom*, dmom*, rung*, ids* and rows handed in as particles
PARTICLES = re.compile(r'\b(?:(?:pos|mom|dmom|rung|ids)(?:_\w+)?|rows)\b')
GATE = re.compile(r'CG_(?:READS_PARTICLES|WRITES_PARTICLES|WRITES_PARTICLES_IF|'
                  r'ADOPTS_PENDING_PASS)\s*\(')
OWN_LINE = re.compile(r'cgk_substep_flush\s*\(|prep_valid\s*=\s*false')
NO_GATE = {
    'cg_substep_begin',      # the pass itself: cgk_substep_begin flushes and voids as it records
    'cg_set_emigrant_rows',  # registers a buffer for later passes, touches no particle
}
OWN_LINE_ALLOWED = {
    'cg_substep_flush',      # the flush as an entry
}


def entries():
    """(name, parameter list, body) of every extern "C" definition in csrc/*.hip"""
    for path in sorted(glob.glob(os.path.join(CSRC, '*.hip'))):
        with open(path, encoding='utf-8') as f:
            text = re.sub(r'//[^\n]*', '', f.read())
        for m in re.finditer(r'extern "C"[^;{(]*?\b(cg_\w+)\s*\(([^)]*)\)\s*\{', text):
            depth, i = 1, m.end()
            while depth:
                depth += {'{': 1, '}': -1}.get(text[i], 0)
                i += 1
            yield m.group(1), m.group(2), text[m.end():i - 1]


def test_every_particle_entry_begins_with_the_gate():
    found = {name: (params, body) for name, params, body in entries()}
    assert len(found) > 100 and NO_GATE | OWN_LINE_ALLOWED <= set(found)
    particle = {name for name, (params, _) in found.items() if PARTICLES.search(params)}
    particle.add('cg_permute_rows')      # (particle columns under the names src and dst)
    assert {'cg_drift', 'cg_lpt_displace', 'cg_shortrange_cells', 'cg_region_insert'} <= particle
    ungated = sorted(name for name in particle - NO_GATE
                     if not GATE.match(found[name][1].lstrip()))
    assert not ungated, f'particle entries that do not begin with a gate line: {ungated}'
    # one gate line, and nothing else of its sort
    twice = sorted(name for name, (_, body) in found.items() if len(GATE.findall(body)) > 1)
    own = sorted(name for name, (_, body) in found.items()
                 if name not in OWN_LINE_ALLOWED and OWN_LINE.search(body))
    assert not twice and not own, (twice, own)
