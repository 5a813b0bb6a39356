"""The kernel census tool (tools/kernel_census.py) on canned symbol lists and canned rocprofv3 CSVs: the matching of traced kernel names
to compiled instantiations, without a GPU -- and the symbol listing on the built library, which holds 1115 instantiations at this commit.

The census itself (the GPU suite module by module under `rocprofv3 --kernel-trace --stats -M --output-format csv -d <dir>/<module> --
python -m pytest -m gpu tests/<module>.py`, then `python tools/kernel_census.py join --symbols build --modules ... -o
profiles/kernel_census.json <dir>/*`) has not been taken yet: no record is committed, and nothing here depends on one."""
import importlib.util
import glob
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('kernel_census', os.path.join(ROOT, 'tools', 'kernel_census.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SYMS = ['_Z10row_kernelILi64ELb0EEvPKfPfi', '_Z10row_kernelILi64ELb1EEvPKfPfi', '_ZN4ktup12_GLOBAL__N_110seg_kernelILi4EEEvPfi',
        '_ZN4ktup11plain_kernelEPfi']


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(text)


def test_join_matches_mangled_and_demangled_names_and_ignores_other_libraries(tmp_path):
    K = _tool()
    # process 1 left a per-dispatch trace with mangled names (rocprofv3 -M), with and without the descriptor suffix
    _write(str(tmp_path / 'a' / 'host' / '11_kernel_trace.csv'),
           '"Kind","Agent_Id","Kernel_Name","Grid_Size"\n'
           '"KERNEL_DISPATCH",1,"_Z10row_kernelILi64ELb0EEvPKfPfi.kd",64\n'
           '"KERNEL_DISPATCH",1,"_Z10row_kernelILi64ELb0EEvPKfPfi",64\n'
           '"KERNEL_DISPATCH",1,"_ZN2at6native18elementwise_kernelILi128ELi4EZNS0_3fooEvEUliE_EEviT1_",64\n')
    # ... and its stats file, which must not be counted on top of the trace
    _write(str(tmp_path / 'a' / 'host' / '11_kernel_stats.csv'),
           '"Name","Calls","TotalDurationNs"\n"_Z10row_kernelILi64ELb0EEvPKfPfi.kd",2,10\n')
    # process 2 left only statistics, with demangled names
    _write(str(tmp_path / 'b' / '12_kernel_stats.csv'),
           '"Name","Calls","TotalDurationNs"\n'
           '"void ktup::(anonymous namespace)::seg_kernel<4>(float*, int)",7,10\n'
           '"void rocprim::detail::sort_kernel<256>(int*)",5,10\n')
    traced = K.read_trace_counts([str(tmp_path / 'a'), str(tmp_path / 'b')])
    per, foreign = K.match_counts(SYMS, traced)
    assert per == {SYMS[0]: 2, SYMS[1]: 0, SYMS[2]: 7, SYMS[3]: 0}
    assert foreign == 6
    ann = {'exempt': {SYMS[3]: 'measurement-only: dbg_eval'}}
    rec = K.make_record(SYMS, per, ['m1', 'm2'], ann, commit='abc')
    assert rec['instantiations'] == 4 and rec['covered'] == 2
    assert rec['cold'] == [SYMS[1]]
    assert rec['exempt'] == [{'symbol': SYMS[3], 'reason': 'measurement-only: dbg_eval'}]
    assert rec['templates']['row_kernel'] == {'instantiations': 2, 'covered': 1}
    assert rec['templates']['seg_kernel'] == {'instantiations': 1, 'covered': 1}
    assert rec['symbols_sha256'] == K.symbols_sha256(list(reversed(SYMS)))            # order-free
    assert rec['symbols_sha256'] != K.symbols_sha256(SYMS + ['_Z10row_kernelILi100ELb0EEvPKfPfi'])


def test_join_fails_loudly_on_a_truncated_or_stale_name(tmp_path):
    K = _tool()
    _write(str(tmp_path / 't' / '1_kernel_stats.csv'), '"Name","Calls"\n"row_kernel",3\n')
    with pytest.raises(K.CensusError, match='match no compiled symbol'):
        K.match_counts(SYMS, K.read_trace_counts([str(tmp_path / 't')]))
    _write(str(tmp_path / 'u' / '1_kernel_stats.csv'), '"Name","Calls"\n"_Z10row_kernelILi999ELb0EEvPKfPfi.kd",3\n')
    with pytest.raises(K.CensusError, match='match no compiled symbol'):
        K.match_counts(SYMS, K.read_trace_counts([str(tmp_path / 'u')]))
    with pytest.raises(K.CensusError, match='no \\*kernel_trace'):
        K.read_trace_counts([str(tmp_path / 'nothing')])
    with pytest.raises(K.CensusError, match='not compiled'):
        K.make_record(SYMS, dict.fromkeys(SYMS, 1), [], {'unreachable': {'_Z3gonev': 'x.hip:1'}})


def test_readelf_parser_keeps_kernel_descriptors_only():
    K = _tool()
    text = ('Symbol table \'.symtab\' contains 4 entries:\n   Num:    Value          Size Type    Bind   Vis       Ndx Name\n'
            '     1: 0000000000001000    64 OBJECT  GLOBAL PROTECTED  7 _Z3fooPf.kd\n'
            '     2: 0000000000002000   512 FUNC    GLOBAL PROTECTED  8 _Z3fooPf\n'
            '     3: 0000000000001040    64 OBJECT  WEAK   PROTECTED  7 _Z3barILi4EEvPf.kd\n')
    assert K.parse_readelf(text) == ['_Z3barILi4EEvPf', '_Z3fooPf']


def test_list_reads_every_kernel_descriptor_of_the_built_objects():
    """`list` on the build: kernel names are unique, every one demangles to a template the report can name, and the two translation
    units without device code (ktup_eval_kg_pass, ktup_runtime) are passed over instead of failing the walk."""
    K = _tool()
    if not K.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf / c++filt not found')
    if not glob.glob(os.path.join(K.OBJECTS, '*.o')):
        pytest.skip('the library is not built (no objects under joint-kg-recommender_amd/build)')
    names = K.list_symbols()
    assert len(names) == len(set(names)) > 0 and all(n.startswith('_Z') for n in names)
    dem = K.demangle(names)
    assert all(K.template_of(x).endswith('kernel') for x in dem), [x for x in dem if not K.template_of(x).endswith('kernel')][:3]
    assert K.symbols_sha256(names) == K.symbols_sha256(sorted(names, reverse=True))
