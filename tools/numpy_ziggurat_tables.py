"""The three 256-entry tables of numpy's ziggurat for the standard exponential distribution
(ke_double, we_double, fe_double of numpy/random/src/distributions/ziggurat_constants.h), read
out of the installed numpy: they are local objects in the .rodata of a member of
numpy/random/lib/libnpyrandom.a.  `ar x` gives the member, `nm -S` the offsets and sizes of the
symbols, `readelf -S` the file offset of .rodata.

  python tools/numpy_ziggurat_tables.py [--out concept_amd/csrc/cg_ziggurat_tables.h]

Run by hand when the header is to be made anew; nothing runs it at build time.  The header holds
the tables as hexadecimal 64-bit literals (the doubles by their bits), under numpy's notice.
tests/test_noise_refs_host.py compares the committed header with what extract() returns."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

NAMES = ('ke_double', 'we_double', 'fe_double')
TOOLS = ('ar', 'nm', 'readelf')

NOTICE = """\
// cg_ziggurat_tables.h — the tables of numpy's ziggurat for the standard exponential
// distribution (ke_double, we_double, fe_double of
// numpy/random/src/distributions/ziggurat_constants.h), as 64-bit words: ke as the integers they
// are, we and fe as the bits of the doubles.  Written by tools/numpy_ziggurat_tables.py from the
// installed numpy; not edited by hand.
//
// Copyright (c) 2005-2024, NumPy Developers.
// All rights reserved.
//
// Redistribution and use in source and binary forms, with or without
// modification, are permitted provided that the following conditions are
// met:
//
//     * Redistributions of source code must retain the above copyright
//        notice, this list of conditions and the following disclaimer.
//
//     * Redistributions in binary form must reproduce the above
//        copyright notice, this list of conditions and the following
//        disclaimer in the documentation and/or other materials provided
//        with the distribution.
//
//     * Neither the name of the NumPy Developers nor the names of any
//        contributors may be used to endorse or promote products derived
//        from this software without specific prior written permission.
//
// THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS
// "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT
// LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR
// A PARTICULAR PURPOSE ARE DISCLAIMED. IN NO EVENT SHALL THE COPYRIGHT
// OWNER OR CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL,
// SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING, BUT NOT
// LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE,
// DATA, OR PROFITS; OR BUSINESS INTERRUPTION) HOWEVER CAUSED AND ON ANY
// THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT
// (INCLUDING NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE
// OF THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
#pragma once
#include <cstdint>
#ifndef CG_ZIG_TABLE  // the qualifiers of the tables: a device file asks for device memory
#define CG_ZIG_TABLE static const
#endif
"""


def missing_tools():
    return [t for t in TOOLS if shutil.which(t) is None]


def extract():
    """{name: list of 256 unsigned 64-bit words} from the installed numpy's libnpyrandom.a"""
    import numpy
    archive = os.path.join(os.path.dirname(numpy.__file__), 'random', 'lib', 'libnpyrandom.a')
    if not os.path.exists(archive):
        raise FileNotFoundError(archive)

    def run(*cmd, **kw):
        return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout

    with tempfile.TemporaryDirectory() as tmp:
        run('ar', 'x', archive, cwd=tmp)
        for member in sorted(os.listdir(tmp)):
            path = os.path.join(tmp, member)
            symbols = {}
            for line in run('nm', '-S', path).splitlines():
                fields = line.split()
                if len(fields) == 4 and fields[3] in NAMES:
                    symbols[fields[3]] = (int(fields[0], 16), int(fields[1], 16))
            if len(symbols) != len(NAMES):
                continue
            # "[ 4] .rodata  PROGBITS  address  offset" and the size on the same or the next line
            sections = run('readelf', '-S', '-W', path)
            m = re.search(r'\]\s+\.rodata\s+PROGBITS\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)',
                          sections)
            if m is None:
                raise RuntimeError(f'no .rodata section in {member}')
            rodata, rodata_size = int(m.group(1), 16), int(m.group(2), 16)
            with open(path, 'rb') as f:
                blob = f.read()
            tables = {}
            for name, (offset, size) in symbols.items():
                if size != 2048 or offset + size > rodata_size:
                    raise RuntimeError(f'{name}: {size} bytes at {offset} of .rodata')
                raw = blob[rodata + offset:rodata + offset + size]
                tables[name] = [int.from_bytes(raw[8*n:8*n + 8], 'little') for n in range(256)]
            return tables
    raise RuntimeError(f'no member of {archive} defines {NAMES}')


def header_text(tables):
    lines = [NOTICE]
    for name in NAMES:
        lines.append(f'CG_ZIG_TABLE uint64_t cg_zig_{name}[256] = {{')
        words = tables[name]
        for n in range(0, 256, 4):
            lines.append('    ' + ' '.join(f'0x{w:016x}ull,' for w in words[n:n + 4]))
        lines.append('};')
    return '\n'.join(lines) + '\n'


def read_header(path):
    """{name: list of 256 words} back from a header this tool wrote"""
    with open(path, 'r', encoding='utf-8') as f:
        text = f.read()
    tables = {}
    for name in NAMES:
        body = re.search(r'cg_zig_%s\[256\] = \{(.*?)\};' % name, text, flags=re.S).group(1)
        tables[name] = [int(w, 16) for w in re.findall(r'0x([0-9a-f]{16})ull', body)]
        if len(tables[name]) != 256:
            raise RuntimeError(f'{path}: {len(tables[name])} entries of {name}')
    return tables


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(here, 'concept_amd', 'csrc',
                                                  'cg_ziggurat_tables.h'))
    args = ap.parse_args()
    if missing_tools():
        sys.exit(f'not found: {", ".join(missing_tools())}')
    with open(args.out, 'w', encoding='utf-8') as f:
        f.write(header_text(extract()))
    print(args.out)


if __name__ == '__main__':
    main()
