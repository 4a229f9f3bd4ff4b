#!/usr/bin/env python3
"""usage: tools/asm_pixel_phase.py <file.s> <kernel-substring> [-v]: the ICP pixel phases of the matching kernels in a hipcc -S listing of track.hip.

A pixel phase is found by its shape, not by labels: it runs from the barrier before the first double-precision conversion of a projection
(`(double)px + 0.5`, kf_project) to the next barrier after the 16-byte model-map gathers that follow it (the reduction's barrier); a kernel
that inlines the phase several times (the loop and its solo finish) gives several.  For each phase: instruction, vector-instruction,
register-move and ds_read counts, the longest run of consecutive v_mov_b64 (a phi-copy ladder) and of v_mov_b32 from one source register
(a re-zeroing block), and -- the point -- its memory operations and waits in order.  -v prints every line of the phase."""
import re
import sys


def kernels(txt):
    for f in re.split(r'\n(?=_Z\w+:)', txt):
        body = f.split('.Lfunc_end', 1)[0]
        yield f.split(':', 1)[0], [l.strip() for l in body.split('\n')
                                   if (l.startswith('\t') and not l.strip().startswith(('.', ';'))) or l.startswith('.LBB')]


def phases(lines):
    bars = [i for i, l in enumerate(lines) if l.startswith('s_barrier')]
    i = 0
    while i < len(lines):
        if lines[i].startswith('v_cvt_f64_f32'):
            lo = max([b for b in bars if b < i], default=0)
            g = [k for k in range(i, min(i + 600, len(lines))) if lines[k].startswith(('global_load_dwordx4', 'global_load_dwordx3'))]
            if len(g) >= 2:                                     # (a projection with no gathers close behind it is another stage's: the cull tail)
                hi = next((b for b in bars if b > g[-1]), len(lines) - 1)
                yield lo, hi
                i = hi
        i += 1


def longest_run(ops, pred):
    best = cur = 0
    for o in ops:
        cur = cur + 1 if pred(o) else 0
        best = max(best, cur)
    return best


def main():
    txt = open(sys.argv[1]).read()
    verbose = '-v' in sys.argv[3:]
    for name, lines in kernels(txt):
        if sys.argv[2] not in name:
            continue
        for n, (lo, hi) in enumerate(phases(lines)):
            body = [l for l in lines[lo:hi + 1] if not l.startswith('.LBB')]
            ops = [l.split()[0] for l in body]
            zero_src = [l.split(',')[-1].strip() if l.startswith('v_mov_b32') and re.fullmatch(r'v\d+|0', l.split(',')[-1].strip()) else None for l in body]
            zrun = best = 0
            for a, b in zip(zero_src, zero_src[1:]):
                zrun = zrun + 1 if a is not None and a == b else 0
                best = max(best, zrun + 1 if zrun else 0)
            print('%s  phase %d  (lines %d..%d)' % (name, n, lo, hi))
            print('  instructions %d  vector %d  moves %d (of them DPP / readlane-free v_mov_b32 %d, v_mov_b64 %d)  ds_read %d  lgkmcnt waits %d  vmcnt waits %d' % (
                len(ops), sum(o.startswith('v_') for o in ops), sum(o.startswith('v_mov') for o in ops),
                sum(o.startswith('v_mov_b32') and 'dpp' not in o for o in ops), sum(o.startswith('v_mov_b64') for o in ops),
                sum(o.startswith('ds_read') for o in ops), sum('lgkmcnt' in l for l in body), sum('vmcnt' in l for l in body)))
            print('  longest v_mov_b64 run %d  longest same-source v_mov_b32 run %d' % (longest_run(ops, lambda o: o.startswith('v_mov_b64')), best))
            for k, l in enumerate(lines[lo:hi + 1]):
                if verbose or 'global_' in l or 'vmcnt' in l or 's_barrier' in l or 's_cbranch' in l or l.startswith('.LBB'):
                    print('  %5d %s' % (lo + k, l))
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', txt, re.S):
        if sys.argv[2] in m.group(1):
            d = dict(re.findall(r'\.(vgpr_count|sgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)', m.group(2)))
            print('%s: %s' % (m.group(1), d))


if __name__ == '__main__':
    main()
