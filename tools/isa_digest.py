#!/usr/bin/env python3
"""One sha256 per device function of the library, for "this refactor must not change one instruction" gates:

    python tools/isa_digest.py [-j N] [-D MACRO ...] [file.hip ...] > after.txt        (default: every realvsr_amd/csrc/*.hip)
    git stash; python tools/isa_digest.py > before.txt; git stash pop; diff before.txt after.txt

Each file is compiled with the Makefile's CXXFLAGS plus `--cuda-device-only -S`; the lines that differ between two compiles of the same
source (`__hip_cuid_*`, `.file`) are dropped.  A symbol's digest covers its body (label .. `.size`), its `.amdhsa_kernel` block and its
entry in the `amdhsa.kernels` metadata, so register counts, LDS / scratch sizes and the kernarg layout are part of it.  The register and
spill columns are printed next to the digest for the cases where a digest is ALLOWED to move.  Needs no GPU; looks for no instruction."""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import shlex
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'realvsr_amd', 'csrc')
META = ('.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size')


def makefile_flags():
    with open(os.path.join(CSRC, 'Makefile')) as f:
        text = f.read()
    var = dict(re.findall(r'^(\w+)\s*\?=\s*(.*)$', text, flags=re.M))
    return shlex.split(re.sub(r'\$\((\w+)\)', lambda m: var[m.group(1)], var['CXXFLAGS']))


def assembly(path, defines):
    cmd = [os.environ.get('HIPCC', 'hipcc')] + makefile_flags() + ['-D' + d for d in defines] + ['--cuda-device-only', '-S', '-o', '-', path]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, cwd=CSRC, universal_newlines=True).stdout
    return [ln for ln in text.splitlines() if '__hip_cuid_' not in ln and not ln.lstrip().startswith('.file')]


def digests(lines):
    """-> {symbol: (sha256 hex, {metadata key: value})}"""
    parts, meta = {}, {}
    sym = None
    for ln in lines:   # function bodies and .amdhsa_kernel blocks
        m = re.match(r'\s*\.type\s+(\S+),@function', ln)
        if m:
            sym = m.group(1)
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            sym = m.group(1)
        if sym is not None:
            parts.setdefault(sym, []).append(ln)
            if re.match(r'\s*\.size\s+%s,' % re.escape(sym), ln) or ln.strip() == '.end_amdhsa_kernel':
                sym = None
    if 'amdhsa.kernels:' in lines:   # metadata: one YAML list item ("  - .agpr_count: ...") per kernel
        item = []
        for ln in lines[lines.index('amdhsa.kernels:') + 1:] + ['  - ']:
            if ln.startswith('  - ') or not ln.startswith('    '):
                name = [x.split(':', 1)[1].strip() for x in item if x.strip().startswith('.name:')]
                if name:
                    parts.setdefault(name[0], []).extend(item)
                    meta[name[0]] = {k: x.split(':', 1)[1].strip() for x in item for k in META if x.strip(' -').startswith(k + ':')}
                item = []
                if not ln.startswith('  - '):
                    break
            item.append(ln)
    return {s: (hashlib.sha256('\n'.join(p).encode()).hexdigest(), meta.get(s, {})) for s, p in parts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('files', nargs='*', help='sources under realvsr_amd/csrc (default: all *.hip)')
    ap.add_argument('-j', type=int, default=4)
    ap.add_argument('-D', action='append', default=[], metavar='MACRO')
    a = ap.parse_args()
    files = sorted(os.path.basename(f) for f in (a.files or glob.glob(os.path.join(CSRC, '*.hip'))))
    with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        for f, lines in zip(files, pool.map(lambda f: assembly(f, a.D), files)):
            for s, (h, m) in sorted(digests(lines).items()):
                print('%s %s %s %s' % (h, f, s, ' '.join('%s=%s' % (k.lstrip('.'), m[k]) for k in META if k in m)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
