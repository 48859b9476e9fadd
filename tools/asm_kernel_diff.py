"""Compare two device-only assembly files kernel by kernel:  python tools/asm_kernel_diff.py before.s after.s

The files come from  hipcc <build.py's flags> -x hip --cuda-device-only -S file.hip -o file.s .  Per kernel: `identical` (same text),
`renumbered` (same opcodes in the same order, same VGPR / SGPR / LDS figures, no scratch: operands differ) or `DIFFERENT`; kernels
that only one file has are listed as `only before` / `only after`.  Exit status 1 unless every kernel is identical or renumbered."""
import re
import subprocess
import sys

FIGURES = ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def kernels(path):
    text = open(path).read()
    body = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        lines = [re.sub(r'\.LBB\d+_', '.LBB_', l.split(';')[0].strip()) for l in m.group(2).split('\n')]     # labels carry the kernel's index in the file
        body[m.group(1)] = [l for l in lines if l and not l.startswith('.') and not l.endswith(':')]
    figures = {}
    for m in re.finditer(r'^\s+- \.agpr_count:.*?^\s+\.wavefront_size:', text, re.S | re.M):
        block = m.group(0)
        name = re.search(r'^\s+\.symbol:\s+(\w+)\.kd', block, re.M).group(1)
        figures[name] = tuple(int(re.search(r'^\s+%s:\s+(\d+)' % re.escape(f), block, re.M).group(1)) for f in FIGURES)
    return {k: (body[k], figures[k]) for k in body if k in figures}


def main(before, after):
    a, b = kernels(before), kernels(after)
    names = subprocess.run(['c++filt'] + sorted(set(a) | set(b)), capture_output=True, text=True).stdout.split('\n')
    ok = True
    for sym, name in zip(sorted(set(a) | set(b)), names):
        name = re.sub(r'^void \(anonymous namespace\)::|\(.*$', '', name)
        if sym not in a or sym not in b:
            state, ok = 'only before' if sym in a else 'only after', False
        elif a[sym] == b[sym]:
            state = 'identical'
        elif [l.split()[0] for l in a[sym][0]] == [l.split()[0] for l in b[sym][0]] and a[sym][1] == b[sym][1] and a[sym][1][3] == 0:
            state = 'renumbered'
        else:
            state, ok = 'DIFFERENT', False
        va, vb = a.get(sym, (0, '-'))[1], b.get(sym, (0, '-'))[1]
        print(f'{name:70s} {state:12s} VGPRs {va[0]} -> {vb[0]}  instructions {len(a.get(sym, [[]])[0])} -> {len(b.get(sym, [[]])[0])}')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
