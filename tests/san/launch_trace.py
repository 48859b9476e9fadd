"""TEST INFRASTRUCTURE: the launch trace of the native library's host halves, per A/B switch.

tests/san/driver.py in trace mode (sanitizer build, the shim recording every kernel launch instead of refusing it) writes which kernel
each of 15876 GEMM problems and each of 170 engine forward passes launches, in which grid, block and dynamic LDS size -- or the error it
answers.  The launchers sample their switches once per process, so `record` runs that mode once per switch, each in a child of its own.
tests/golden/launch_trace.json is `compact(record(lib))` of the commit before gemm.hip's routing became one function
(`python tests/san/launch_trace.py OUT.json` writes it); tests/test_sanitized_host.py requires `expand` of it back from the present code.

Compact form: `names` (kernel names), `launches` ([name, grid x y z, block x y z, LDS bytes]) and `outcomes` ([return code, error text,
[launches]]) are tables of distinct values, each indexing the one before; a run is a list of outcome indices for the GEMM grid (in the
driver's enumeration order) and a map sequence -> outcome index for the engine.  The run without a switch is stored whole, the others as
their differences from it."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ('', 'AMTX_GEMM_NO_SKINNY', 'AMTX_GEMM_NO_PP', 'AMTX_GEMM_PP', 'AMTX_GEMM_NO_SPLIT_DMA', 'AMTX_NO_CONVX', 'AMTX_CONVG_NO_STRIP')
# every switch a launcher or the engine reads: none of them may leak in from the caller's environment
ALL_SWITCHES = SWITCHES[1:] + ('AMTX_NO_CONVG_MC2', 'AMTX_NO_CONV_FUSE', 'AMTX_X3_NO_SPLIT', 'AMTX_NO_CONVX12M', 'AMTX_OF_ROWMAJOR_A3', 'AMTX_OF_NO_ROLL_EPILOGUE',
                               'AMTX_CONVG_NO_WDMA', 'AMTX_CONVG_NO_CSPLIT', 'AMTX_LSTM_NO8', 'AMTX_CONVF_DBG')


def record(lib, san_env):
    """{switch: {'gemm': [outcome ...], 'engine': {sequence: outcome}}}, outcome = [rc, error, ['name<tab>grid block lds' ...]]; the
    children run side by side."""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for i, switch in enumerate(SWITCHES):
            env = {k: v for k, v in san_env.items() if k not in ALL_SWITCHES}
            if switch:
                env[switch] = '1'
            out = os.path.join(tmp, '%d.json' % i)
            procs.append((switch, out, subprocess.Popen([sys.executable, os.path.join(HERE, 'driver.py'), lib, '-', out], env=env,
                                                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        runs = {}
        for switch, out, p in procs:
            stdout, stderr = p.communicate(timeout=900)
            assert p.returncode == 0, (switch, stdout[-2000:], stderr[-6000:])
            with open(out) as f:
                runs[switch] = json.load(f)
    return runs


def compact(runs):
    tables = {'names': {}, 'launches': {}, 'outcomes': {}}

    def index(table, value):
        return tables[table].setdefault(json.dumps(value), len(tables[table]))

    def outcome(o):
        launches = []
        for line in o[2]:
            name, nums = line.split('\t')
            launches.append(index('launches', [index('names', name)] + [int(x) for x in nums.split()]))
        return index('outcomes', [o[0], o[1], launches])
    ids = {s: {'gemm': [outcome(o) for o in r['gemm']], 'engine': {k: outcome(o) for k, o in r['engine'].items()}} for s, r in runs.items()}
    base, out = ids[''], {}
    for s, r in ids.items():
        assert len(r['gemm']) == len(base['gemm']) and list(r['engine']) == list(base['engine'])
        out[s] = r if not s else {'gemm_differs': [[i, o] for i, (o, b) in enumerate(zip(r['gemm'], base['gemm'])) if o != b],
                                  'engine_differs': {k: o for k, o in r['engine'].items() if o != base['engine'][k]}}
    return dict({t: [json.loads(k) for k in v] for t, v in tables.items()}, runs=out)


def expand(c):
    """The inverse of compact."""
    def outcome(i):
        rc, err, launches = c['outcomes'][i]
        return [rc, err, ['%s\t%s' % (c['names'][l[0]], ' '.join(str(x) for x in l[1:])) for l in (c['launches'][j] for j in launches)]]
    runs = {}
    for s, r in c['runs'].items():
        gemm, engine = list(c['runs']['']['gemm']), dict(c['runs']['']['engine'])
        if s:
            for i, o in r['gemm_differs']:
                gemm[i] = o
            engine.update(r['engine_differs'])
        runs[s] = {'gemm': [outcome(i) for i in gemm], 'engine': {k: outcome(i) for k, i in engine.items()}}
    return runs


def write(c, path):
    with open(path, 'w') as f:
        f.write('{' + ',\n'.join('"%s": [\n%s\n]' % (t, ',\n'.join(json.dumps(v) for v in c[t])) for t in ('names', 'launches', 'outcomes')) +
                ',\n"runs": {\n' + ',\n'.join('%s: %s' % (json.dumps(s), json.dumps(r)) for s, r in c['runs'].items()) + '\n}}\n')


if __name__ == '__main__':
    import build_san
    env = dict(os.environ, LD_PRELOAD=build_san.asan_runtime(), ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    got = compact(record(build_san.build(), env))
    assert expand(got) == expand(json.loads(json.dumps(got)))
    write(got, sys.argv[1])
