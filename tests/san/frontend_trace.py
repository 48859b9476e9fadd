"""TEST INFRASTRUCTURE: the launch trace of the front-end's host halves (spec.hip, cqt.hip, cqt_dec.hip and the GEMM route they take through
gemm.hip), per A/B switch.

tests/san/frontend_trace.cpp -- a stand-alone program linked with the sanitizer build of the host halves and the recording shim -- reads the
case list `cases()` makes and prints, per case, the return code, the error text and every kernel launch (name, grid, block, dynamic LDS
bytes).  The launchers sample their switches once per process, so `record` runs the program once per switch, each in a child of its own.
tests/golden/frontend_trace.json is `compact(record())` of the commit before the front-end's launch decisions became one route per file
(`python tests/san/frontend_trace.py OUT.json` writes it); tests/test_frontend_trace.py requires `expand` of it back from the present code.

Compact form, as in tests/san/launch_trace.py: `names`, `launches` ([name, numbers ...]) and `outcomes` ([return code, error text,
[launches]]) are tables of distinct values, each indexing the one before (a launch list that repeats a block is folded, `_fold`); a run is a
list of outcome indices in the order of `cases()`, whose SHA-256 the file carries.  The run without a switch is stored whole, the others as
their differences from it."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

SWITCHES = ('', 'AMTX_SPEC_NO_RING', 'AMTX_CQT_COPY_LEVEL0', 'AMTX_CQT_GEMM_BASIS', 'AMTX_CQT_DECIM_V1', 'AMTX_CQT_DECIM_BLOCKS=64')
# every switch the front-end or the GEMM launcher behind it reads: none of them may leak in from the caller's environment
ALL_SWITCHES = ('AMTX_SPEC_NO_RING', 'AMTX_SPEC_NATURAL_ROWS', 'AMTX_CQT_COPY_LEVEL0', 'AMTX_CQT_GEMM_BASIS', 'AMTX_CQT_DECIM_V1', 'AMTX_CQT_DECIM_BLOCKS',
                'AMTX_GEMM_NO_SKINNY', 'AMTX_GEMM_NO_PP', 'AMTX_GEMM_PP', 'AMTX_GEMM_NO_SPLIT_DMA')

# (sample rate, n_fft, hop, n_mels, center, pad mode): the kernel each should reach, with the tap slots amtx_spec_mel_layout answers
SPEC_PLANS = (
    (22050, 2048, 512, 229, 1, 0),      # ring (tap slots 4 + 8 + 20 + 32)
    (22050, 2048, 256, 229, 1, 0),      # general, mel weights in LDS: the ring's layout at another hop (64 slots)
    (22050, 2048, 512, 128, 1, 0),      # general, mel weights in LDS (68 slots)
    (22050, 2048, 512, 64, 1, 0),       # general, mel weights from memory (104 slots > MEL_LDS_MAX_SLOTS = 80)
    (22050, 2048, 512, 0, 1, 0),        # general, no mel stage
    (16000, 1024, 256, 80, 1, 0),       # pow2 with mel
    (22050, 128, 32, 0, 1, 0),          # pow2, smallest frame
    (22050, 4096, 1024, 0, 1, 0),       # pow2, largest frame
    (22050, 2048, 512, 229, 0, 0),      # not centred
    (22050, 2048, 512, 229, 1, 1),      # reflecting pad
)
SPEC_GRID_TOO_LARGE = (65535, 1048600)       # x hop samples: 32769 chunks of 32 frames x 65535 clips >= 2^31


def spec_sizes(n_fft, hop):
    return ((1, n_fft // 2 + 1), (2, 512 * 9), (3, 5000), (5, 512 * 40 + 13), (1024, 320000), (SPEC_GRID_TOO_LARGE[0], SPEC_GRID_TOO_LARGE[1] * hop))


def cqt_configs():
    """(name, configuration): every plan of cqt_ref.PLANS at each librosa version it lists, CQT 84 / 12 (the sweep's), BASELINE config 3's
    HCQT, nine harmonics on the windowed route (the 16-bit clip forms refuse it) and a VQT whose levels mix n_fft 256 and 128 (256 256 128 128:
    both windowed kernels in one call; no plan of cqt_ref.PLANS does)."""
    import cqt_ref
    out = [('cqt84', cqt_ref.cfg(84, 12)), ('hcqt72', cqt_ref.cfg(72, 12, harmonics=cqt_ref.HCQT_DEFAULT)),
           ('hcqt-9', cqt_ref.cfg(48, 12, harmonics=(0.5,) + tuple(range(1, 9)))), ('vqt-gamma2', cqt_ref.cfg(48, 12, gamma=2.0)),
           ('vqt-gamma2-lv09', cqt_ref.cfg(48, 12, gamma=2.0, lv='0.9'))]
    for name, c, _, _, route09 in cqt_ref.PLANS:
        out.append((name, c))
        if route09:
            out.append((name + '-lv09', dict(c, lv='0.9')))
    return out


def cases():
    """The one case list: lines of tests/san/frontend_trace.cpp's grammar."""
    import cqt_ref
    lines = []
    for sr, n_fft, hop, n_mels, center, pad in SPEC_PLANS:
        plan = '%d %d %d %d %d %d' % (sr, n_fft, hop, n_mels, center, pad)
        if n_mels:
            lines.append('spec mel_layout %s 1 0' % plan)
        for batch, n in spec_sizes(n_fft, hop):
            lines.append('spec power %s %d %d' % (plan, batch, n))
            lines.append('spec power_clips %s %d %d' % (plan, batch, 1 + n // hop))
    for name, c in cqt_configs():
        hs = sorted(c['harmonics'])
        plan = '%d %d %d %d %r %d %d %r %d %s' % (c['lv'] == '0.9', len(hs) > 1, c['sr'], c['hop'], c['fmin'], c['n_bins'], c['bpo'], c['gamma'], len(hs),
                                                 ' '.join(repr(h) for h in hs))
        lengths = [cqt_ref.PLAN_N]
        if name == 'cqt84':
            lengths += list(cqt_ref.SWEEP)
        if name in ('cqt84', 'hcqt72'):
            lengths.append(9 * c['sr'])
        if c['lv'] == '0.9':
            lengths += [cqt_ref.min_reflect_samples(c), cqt_ref.min_reflect_samples(c) - 1]
        for n in lengths:
            for entry in ('num_frames', 'track_layout'):
                lines.append('cqt %s %s 1 %d' % (entry, plan, n))
            for batch in (1, 3, 512):
                for entry in ('workspace_bytes', 'clips_workspace_bytes', 'forward', 'forward16', 'forward16_split', 'power_clips', 'clips', 'clips16',
                              'clips16_split'):
                    lines.append('cqt %s %s %d %d' % (entry, plan, batch, n))
                # a bank of 512 tracks is 512 chains: only the two flagship plans, at one length
                if batch < 512 or (name in ('cqt84', 'hcqt72') and n == cqt_ref.PLAN_N):
                    lines.append('cqt pyramid_build %s %d %d' % (plan, batch, n))
        for entry in ('forward_small_ws', 'clips_small_ws'):
            lines.append('cqt %s %s 3 %d' % (entry, plan, cqt_ref.PLAN_N))
    return lines


def parse(stdout):
    """[[return code, error text, ['name<tab>numbers' ...]] per case]"""
    out = []
    lines = stdout.split('\n')
    assert lines[-2:] == ['done', ''], lines[-3:]
    for line in lines[:-2]:
        if line.startswith('=\t'):
            _, rc, err = line.split('\t', 2)
            out.append([int(rc), err, []])
        else:
            out[-1][2].append(line)
    return out


def record(exe=None):
    """{switch: [outcome per case]}; the children run side by side; a report of either sanitizer ends a child with an error (the options of tests/test_sanitized_host.py)."""
    import build_san
    exe = exe or build_san.build_program('frontend_trace')
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'cases.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(cases()) + '\n')
        procs = []
        for switch in SWITCHES:
            env = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
            env.update(ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
            if switch:
                name, _, value = switch.partition('=')
                env[name] = value or '1'
            procs.append((switch, subprocess.Popen([exe, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        runs = {}
        for switch, p in procs:
            stdout, stderr = p.communicate(timeout=900)
            assert p.returncode == 0 and 'runtime error' not in stderr and 'AddressSanitizer' not in stderr, (switch, p.returncode, stdout[-2000:], stderr[-6000:])
            runs[switch] = parse(stdout)
            assert len(runs[switch]) == len(cases()), (switch, len(runs[switch]))
    return runs


def cases_sha256():
    import hashlib
    return hashlib.sha256('\n'.join(cases()).encode()).hexdigest()


def _fold(ids):
    """A list that begins with k >= 3 repetitions of a block of at most 64 entries (the chains of a large bank) as {'rep': k, 'of': block,
    'then': rest}; any other list as it is."""
    best = None
    for p in range(1, min(64, len(ids) // 3) + 1):
        k = 1
        while ids[p * k:p * (k + 1)] == ids[:p]:
            k += 1
        if k >= 3 and (best is None or p * k > best[0] * best[1]):
            best = (p, k)
    return ids if best is None else {'rep': best[1], 'of': ids[:best[0]], 'then': ids[best[0] * best[1]:]}


def _unfold(ids):
    return ids['of'] * ids['rep'] + ids['then'] if isinstance(ids, dict) else ids


def compact(runs, sha256=None):
    """`sha256`: that of the case list the runs are of, where it is not `cases()` (tests/san/train_trace.py)."""
    tables = {'names': {}, 'launches': {}, 'outcomes': {}}

    def index(table, value):
        return tables[table].setdefault(json.dumps(value), len(tables[table]))

    def outcome(o):
        launches = []
        for line in o[2]:
            name, nums = line.split('\t')
            launches.append(index('launches', [index('names', name)] + [int(x) for x in nums.split()]))
        return index('outcomes', [o[0], o[1], _fold(launches)])
    ids = {s: [outcome(o) for o in r] for s, r in runs.items()}
    base = ids['']
    out = {s: r if not s else [[i, o] for i, (o, b) in enumerate(zip(r, base)) if o != b] for s, r in ids.items()}
    return dict({t: [json.loads(k) for k in v] for t, v in tables.items()}, cases_sha256=sha256 or cases_sha256(), runs=out)


def expand(c):
    """The inverse of compact: {switch: [outcome per case]}, in the order of cases()."""
    def outcome(i):
        rc, err, launches = c['outcomes'][i]
        return [rc, err, ['%s\t%s' % (c['names'][l[0]], ' '.join(str(x) for x in l[1:])) for l in (c['launches'][j] for j in _unfold(launches))]]
    runs = {}
    for s, r in c['runs'].items():
        ids = list(c['runs'][''])
        if s:
            for i, o in r:
                ids[i] = o
        runs[s] = [outcome(i) for i in ids]
    return runs


def write(c, path):
    """Valid JSON with several table rows to a line; a 'parent_commit' entry goes into the header next to the case list's hash."""
    def rows(values):
        lines, line = [], ''
        for v in (json.dumps(v, separators=(',', ':')) for v in values):
            if line and len(line) + len(v) > 180:
                lines.append(line)
                line = ''
            line += (',' if line else '') + v
        return ',\n'.join(lines + [line])
    with open(path, 'w') as f:
        f.write('{' + ',\n'.join('"%s": [\n%s\n]' % (t, rows(c[t])) for t in ('names', 'launches', 'outcomes')) +
                ',\n"cases_sha256": "%s",\n' % c['cases_sha256'] + ('"parent_commit": "%s",\n' % c['parent_commit'] if 'parent_commit' in c else '') + '"runs": {\n' +
                ',\n'.join('%s: [\n%s\n]' % (json.dumps(s), rows(r)) for s, r in c['runs'].items()) + '\n}}\n')


if __name__ == '__main__':
    got = compact(record())
    assert expand(got) == expand(json.loads(json.dumps(got)))
    write(got, sys.argv[1])
