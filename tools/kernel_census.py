"""Kernel census: which compiled gfx950 kernel instantiations does the GPU suite launch?

    python tools/kernel_census.py list [--objects DIR] [--demangle]          # mangled kernel symbols of the built objects, one per line
    python tools/kernel_census.py join --symbols FILE|build --modules a,b,c [--annotations FILE] [--commit SHA] -o RECORD.json TRACE_DIR ...
    python tools/kernel_census.py report BEFORE.json AFTER.json              # per-template coverage of two records, as a markdown table

`list` walks joint-kg-recommender_amd/build/*.o: llvm-objcopy dumps each object's .hip_fatbin, clang-offload-bundler unbundles the
gfx950 code object, llvm-readelf lists its symbols and the names that end in `.kd` (kernel descriptors) are the kernels.  (The linked
.so concatenates one bundle per translation unit and the bundler reads only the first: hence the objects.)

`join` reads the output directories of `rocprofv3 --kernel-trace [--stats] --output-format csv` runs (every *kernel_trace.csv and
*kernel_stats.csv below them, one per traced process) and writes the record: dispatch counts folded into covered / cold /
exempt / unreachable.  Traced names are matched as mangled names when the profiler printed them (`-M`), else both sides are demangled
by the same c++filt.  A traced name that looks like one of the library's kernels but matches no symbol is an ERROR: a truncated name
would otherwise read as a coverage gap.  Kernels of other libraries (torch, rocPRIM, RCCL) are counted and ignored.

The annotations file (JSON) holds {"exempt": {mangled: reason}, "unreachable": {mangled: reason}}: symbols that are allowed to be cold.

The record is meant for profiles/kernel_census.json (commit, instantiations, symbols_sha256, traced modules, covered count, the full
mangled names of cold / exempt / unreachable, coverage per template): kilobytes, keyed on names so that editing a kernel's body does
not invalidate it while adding or removing an instantiation does.
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = os.path.join(ROOT, 'joint-kg-recommender_amd', 'build')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
LLVM_DIRS = [os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin'), os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')]


class CensusError(Exception):
    pass


def find_tool(name):
    for d in LLVM_DIRS:
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def tools_available():
    return all(find_tool(t) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')) and shutil.which('c++filt') is not None


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise CensusError('%s failed:\n%s' % (' '.join(cmd), r.stderr))
    return r.stdout


def object_symbols(obj, tmp):
    """Mangled kernel names (without .kd) of one host object's gfx950 code object; [] when it carries no device code."""
    fat = os.path.join(tmp, os.path.basename(obj) + '.fatbin')
    co = os.path.join(tmp, os.path.basename(obj) + '.co')
    if '.hip_fatbin' not in _run([find_tool('llvm-readelf'), '-SW', obj]):        # host-only translation unit
        return []
    _run([find_tool('llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, obj, os.path.join(tmp, 'discard.o')])
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return []
    targets = _run([find_tool('clang-offload-bundler'), '--list', '--type=o', '--input=' + fat]).split()
    if TARGET not in targets:
        return []
    _run([find_tool('clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET, '--input=' + fat, '--output=' + co])
    if os.path.getsize(co) == 0:
        return []
    return parse_readelf(_run([find_tool('llvm-readelf'), '-sW', co]))


def parse_readelf(text):
    """Names ending in .kd out of `llvm-readelf -sW` output (the name is the last column)."""
    names = set()
    for line in text.splitlines():
        parts = line.split()
        if len(parts) >= 8 and parts[-1].endswith('.kd') and parts[3] == 'OBJECT':
            names.add(parts[-1][:-3])
    return sorted(names)


def list_symbols(objects=OBJECTS):
    objs = sorted(glob.glob(os.path.join(objects, '*.o')))
    if not objs:
        raise CensusError('no objects under %s: build the library first' % objects)
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            names.update(object_symbols(o, tmp))
    return sorted(names)


def symbols_sha256(names):
    return hashlib.sha256('\n'.join(sorted(names)).encode()).hexdigest()


def demangle(names):
    names = list(names)
    if not names:
        return []
    r = subprocess.run(['c++filt'], input='\n'.join(names) + '\n', capture_output=True, text=True)
    if r.returncode != 0:
        raise CensusError('c++filt failed: ' + r.stderr)
    out = r.stdout.split('\n')[:len(names)]
    if len(out) != len(names):
        raise CensusError('c++filt returned %d names for %d' % (len(out), len(names)))
    return out


def template_of(demangled):
    """`void ktup::(anonymous namespace)::row_kernel<...>(...)` -> `row_kernel`."""
    s = demangled.replace('(anonymous namespace)::', '')
    if s.startswith('void '):
        s = s[5:]
    cut = min([k for k in (s.find('<'), s.find('(')) if k >= 0] or [len(s)])
    return s[:cut].split('::')[-1]


def read_trace_counts(dirs):
    """{traced kernel name: dispatches} over every *kernel_trace.csv (one row per dispatch) and *kernel_stats.csv (Name, Calls) below
    `dirs`; a process that left both is counted from its trace."""
    counts = {}
    n_files = 0
    for d in dirs:
        traces = sorted(glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True))
        stats = sorted(glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True))
        have_trace = set(t[:-len('kernel_trace.csv')] for t in traces)
        for path in traces:
            n_files += 1
            with open(path, newline='') as f:
                for row in csv.DictReader(f):
                    name = row.get('Kernel_Name')
                    if name is None:
                        raise CensusError('%s has no Kernel_Name column' % path)
                    counts[name] = counts.get(name, 0) + 1
        for path in stats:
            if path[:-len('kernel_stats.csv')] in have_trace:
                continue
            n_files += 1
            with open(path, newline='') as f:
                for row in csv.DictReader(f):
                    if 'Name' not in row or 'Calls' not in row:
                        raise CensusError('%s has no Name / Calls columns' % path)
                    counts[row['Name']] = counts.get(row['Name'], 0) + int(row['Calls'])
    if n_files == 0:
        raise CensusError('no *kernel_trace.csv or *kernel_stats.csv under ' + ', '.join(dirs))
    return counts


def _norm(name):
    name = name.strip()
    if name.endswith('.kd'):
        name = name[:-3]
    if name.endswith(' [clone .kd]'):
        name = name[:-len(' [clone .kd]')]
    return name


def match_counts(symbols, traced, demangler=demangle):
    """-> ({mangled symbol: dispatches}, dispatches of other libraries).  A traced name is the library's when it equals a symbol
    (mangled, or demangled on both sides) -- and when it merely shares a kernel's base name without matching any instantiation, that
    is an error, not a kernel of somebody else."""
    per = dict.fromkeys(symbols, 0)
    rest = {}
    for raw, n in traced.items():
        name = _norm(raw)
        if name in per:
            per[name] += n
        else:
            rest[name] = rest.get(name, 0) + n
    foreign, unmatched = 0, []
    if rest:
        dem_syms = [_norm(s) for s in demangler(symbols)]
        by_dem = dict(zip(dem_syms, symbols))
        own = set(template_of(d) for d in dem_syms)
        names = list(rest)
        mangled = [k for k in names if k.startswith('_Z')]
        dem = dict(zip(mangled, demangler(mangled)))
        for name in names:
            d = _norm(dem.get(name, name))
            if d in by_dem:
                per[by_dem[d]] += rest[name]
            elif template_of(d) in own:
                unmatched.append(name)
            else:
                foreign += rest[name]
    if unmatched:
        raise CensusError('%d traced kernel name(s) of the library match no compiled symbol (truncated names? stale build?), e.g.\n  %s'
                          % (len(unmatched), '\n  '.join(sorted(unmatched)[:5])))
    return per, foreign


def make_record(symbols, per, modules, annotations=None, commit='', notes=None, demangler=demangle):
    annotations = annotations or {}
    exempt, unreachable = annotations.get('exempt', {}), annotations.get('unreachable', {})
    for kind, d in (('exempt', exempt), ('unreachable', unreachable)):
        stray = sorted(set(d) - set(symbols))
        if stray:
            raise CensusError('%s annotation names a symbol that is not compiled: %s' % (kind, stray[0]))
    covered = [s for s in symbols if per[s] > 0]
    cold_all = [s for s in symbols if per[s] == 0]
    cold = [s for s in cold_all if s not in exempt and s not in unreachable]
    templates = {}
    for s, dm in zip(symbols, demangler(symbols)):
        t = templates.setdefault(template_of(dm), [0, 0])
        t[0] += 1
        t[1] += per[s] > 0
    return {
        'commit': commit,
        'instantiations': len(symbols),
        'symbols_sha256': symbols_sha256(symbols),
        'modules': list(modules),
        'covered': len(covered),
        'cold': cold,
        'exempt': [{'symbol': s, 'reason': exempt[s]} for s in cold_all if s in exempt],
        'unreachable': [{'symbol': s, 'reason': unreachable[s]} for s in cold_all if s in unreachable],
        'templates': {k: {'instantiations': v[0], 'covered': v[1]} for k, v in sorted(templates.items())},
        'notes': notes or [],
    }


def report(before, after):
    """Markdown table of two records: instantiations and covered ones per template, before and after."""
    lines = ['| template | instantiations | covered before | covered after |', '|---|---|---|---|']
    tb, ta = before['templates'], after['templates']
    for k in sorted(ta, key=lambda k: (-ta[k]['instantiations'], k)):
        b = tb.get(k, {'covered': 0})['covered']
        if b < ta[k]['instantiations'] or ta[k]['covered'] < ta[k]['instantiations']:
            lines.append('| `%s` | %d | %d | %d |' % (k, ta[k]['instantiations'], b, ta[k]['covered']))
    full = sum(1 for k in ta if tb.get(k, {'covered': 0})['covered'] == ta[k]['instantiations'] == ta[k]['covered'])
    lines.append('| %d templates covered in full by both | | | |' % full)
    lines.append('| **all** | **%d** | **%d** | **%d** |' % (after['instantiations'], before['covered'], after['covered']))
    return '\n'.join(lines)


def _load_symbols(arg):
    if arg == 'build':
        return list_symbols()
    with open(arg) as f:
        return sorted(set(l.strip() for l in f if l.strip()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    ls = sub.add_parser('list')
    ls.add_argument('--objects', default=OBJECTS)
    ls.add_argument('--demangle', action='store_true')
    jn = sub.add_parser('join')
    jn.add_argument('--symbols', default='build', help="a file of mangled names, or 'build' to read the built objects")
    jn.add_argument('--modules', default='', help='comma-separated names of the traced test modules')
    jn.add_argument('--annotations')
    jn.add_argument('--commit', default='')
    jn.add_argument('--note', action='append', default=[])
    jn.add_argument('--counts', help='also write {symbol: dispatches} here (large; not for the repository)')
    jn.add_argument('-o', '--output', required=True)
    jn.add_argument('dirs', nargs='+')
    rp = sub.add_parser('report')
    rp.add_argument('before')
    rp.add_argument('after')
    a = ap.parse_args(argv)
    try:
        if a.cmd == 'report':
            print(report(json.load(open(a.before)), json.load(open(a.after))))
            return 0
        if a.cmd == 'list':
            names = list_symbols(a.objects)
            for n in (demangle(names) if a.demangle else names):
                print(n)
            print('%d kernel instantiations, sha256 %s' % (len(names), symbols_sha256(names)), file=sys.stderr)
            return 0
        symbols = _load_symbols(a.symbols)
        per, foreign = match_counts(symbols, read_trace_counts(a.dirs))
        ann = json.load(open(a.annotations)) if a.annotations else None
        rec = make_record(symbols, per, [m for m in a.modules.split(',') if m], ann, a.commit, a.note)
        with open(a.output, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
        if a.counts:
            with open(a.counts, 'w') as f:
                json.dump(per, f, indent=0)
        print('%d instantiations, %d covered, %d cold, %d exempt, %d unreachable (%d dispatches of other libraries ignored)'
              % (len(symbols), rec['covered'], len(rec['cold']), len(rec['exempt']), len(rec['unreachable']), foreign))
        return 0
    except CensusError as e:
        print('kernel_census: ' + str(e), file=sys.stderr)
        return 2


if __name__ == '__main__':
    sys.exit(main())
