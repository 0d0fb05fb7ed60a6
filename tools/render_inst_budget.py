"""Static instruction budget of the fused ray-marcher's forward kernels (csrc/render.hip, csrc/render_device.h).

Compiles render.hip to gfx950 assembly with the flags of pix2pix3d_amd/build.py (no GPU needed) and prints, for every
render_forward_kernel instantiation, the registers / spills / scratch the compiler reports and, for every loop of the kernel
that holds matrix instructions, the instruction classes of one trip:

    VALU    every v_* instruction that is not an MFMA (the two columns after it are subsets of this one)
    trans   v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos
    pk      v_pk_*
    MFMA    v_mfma_*
    LDS     ds_*        VMEM  buffer_* / global_* / flat_* / scratch_*
    s_nop, scalar branches (s_branch / s_cbranch_*), other SALU, s_waitcnt

A loop is found from the control-flow graph of the basic blocks (a branch to a block that dominates it).  Inside a loop the wave
branches over blocks — the softplus slow path, the first sample's skipped interval, lanes masked off a store — so a loop gets
three kinds of rows: the sum over EVERY block of its body, the way through it that issues the fewest vector instructions, and,
one row each, the larger blocks that way does not pass (a wave-step's real count is the first row minus the rows of the blocks
it did not enter: in the new kernels, minus the softplus slow paths).  The loops with MFMAs are, in program order, phase A
(coarse densities) and phase C (merged decode + composite); phase B's scans hold no MFMA and are listed, like the loops around
these, with --all.

It counts instruction classes and nothing else: no timing, no model of the issue logic.

    python tools/render_inst_budget.py [--all] [--keep-asm PATH]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRANS = ('v_exp_', 'v_log_', 'v_rcp_', 'v_rsq_', 'v_sqrt_', 'v_sin_', 'v_cos_')
CLASSES = ['VALU', 'trans', 'pk', 'MFMA', 'LDS', 'VMEM', 's_nop', 'branch', 'SALU', 'waitcnt']


def classify(op):
    """Instruction mnemonic -> list of the classes it counts in."""
    if op.startswith('v_mfma') or op.startswith('v_smfmac'):
        return ['MFMA']
    if op.startswith('v_'):
        c = ['VALU']
        if op.startswith(TRANS):
            c.append('trans')
        if op.startswith('v_pk_'):
            c.append('pk')
        return c
    if op.startswith('ds_'):
        return ['LDS']
    if op.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
        return ['VMEM']
    if op == 's_nop':
        return ['s_nop']
    if op in ('s_branch', 's_setpc_b64') or op.startswith('s_cbranch'):
        return ['branch']
    if op.startswith('s_waitcnt') or op == 's_barrier':
        return ['waitcnt']
    if op.startswith('s_'):
        return ['SALU']
    return []


def compile_asm(out_path):
    from pix2pix3d_amd import build
    src = os.path.join(build.CSRC, 'render.hip')
    cmd = [build._hipcc()] + build.CXXFLAGS + ['--cuda-device-only', '-S', src, '-o', out_path]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed:\n{r.stdout}')


def demangle(names):
    try:
        r = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, text=True, check=True)
        return r.stdout.split('\n')[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return names


def parse_functions(text):
    """symbol -> [body lines, {resource: value} from the comments the compiler puts behind the function]."""
    funcs, name = {}, None
    for line in text.split('\n'):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            name = m.group(1)
            funcs[name] = [[], {}, False]
            continue
        if name is None:
            continue
        if line.startswith('.Lfunc_end'):
            funcs[name][2] = True
        elif not funcs[name][2]:
            funcs[name][0].append(line)
        else:
            m = re.match(r'^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|NumSgprs|LDSByteSize): (\d+)', line)
            if m:
                funcs[name][1][m.group(1)] = int(m.group(2))
    return {k: v[:2] for k, v in funcs.items()}


def kernel_metadata(text):
    """Per-kernel metadata entries ('.name' .. next '- .agpr_count' item) -> {symbol: {key: value}}."""
    out = {}
    start = text.find('amdhsa.kernels:')
    if start < 0:
        return out
    for item in re.split(r'\n  - ', text[start:])[1:]:
        kv = dict(re.findall(r'\n?\s*\.(\w+):\s+(\S+)', '\n' + item))
        if 'symbol' in kv:
            out[kv['symbol'].replace('.kd', '')] = kv
    return out


def blocks_of(body):
    """[[label or None, [(mnemonic, branch target or None)]]] in layout order, and label -> block index."""
    blocks, index = [[None, []]], {}
    for line in body:
        m = re.match(r'^(\.LBB\d+_\d+):', line)
        if m:
            blocks.append([m.group(1), []])
            index[m.group(1)] = len(blocks) - 1
            continue
        if re.match(r'^; %bb\.\d+:', line):                # a block that is only fallen into carries no label
            blocks.append([None, []])
            continue
        s = line.strip()
        if not s or s.startswith((';', '.', '//')):
            continue
        parts = s.split()
        op = parts[0]
        target = None
        if op == 's_branch' or op.startswith('s_cbranch'):
            target = parts[1].rstrip(',') if len(parts) > 1 else None
        blocks[-1][1].append((op, target))
    return blocks, index


def count_block(insts):
    c = dict.fromkeys(CLASSES, 0)
    for op, _ in insts:
        for k in classify(op):
            c[k] += 1
    return c


def add(a, b):
    return {k: a[k] + b[k] for k in CLASSES}


def successors(blocks, index):
    """Block -> blocks it can continue in: branch targets, and the next block unless it ends in s_branch / s_endpgm."""
    succ = []
    for i, (_, insts) in enumerate(blocks):
        s = [index[tgt] for _, tgt in insts if tgt is not None and tgt in index]
        if not (insts and insts[-1][0] in ('s_branch', 's_endpgm', 's_setpc_b64')) and i + 1 < len(blocks):
            s.append(i + 1)
        succ.append(sorted(set(s)))
    return succ


def loops_of(blocks, index, succ):
    """head block -> (tails, body): the blocks that branch back to the head, and every block on a way from the head to one of them."""
    pred = [[] for _ in blocks]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)
    n = len(blocks)
    dom = [{0}] + [set(range(n)) for _ in range(n - 1)]   # dominators, iterated to the fixed point: a back edge is t -> h with h dominating t
    changed = True
    while changed:
        changed = False
        for i in range(1, n):
            ps = [dom[q] for q in pred[i]]
            d = (set.intersection(*ps) if ps else set()) | {i}
            if d != dom[i]:
                dom[i], changed = d, True
    tails = {}
    for t, ss in enumerate(succ):
        for h in ss:
            if h in dom[t]:
                tails.setdefault(h, set()).add(t)
    loops = {}
    for h, ts in tails.items():
        body, todo = {h}, [t for t in ts if t != h]
        while todo:                                       # backwards from the tails, not through the head
            i = todo.pop()
            if i in body:
                continue
            body.add(i)
            todo.extend(pred[i])
        fwd, todo = set(), [h]
        while todo:                                       # forwards from the head, not back through it
            i = todo.pop()
            if i in fwd:
                continue
            fwd.add(i)
            todo.extend(j for j in succ[i] if j != h)
        ts = {t for t in ts if t in fwd}                  # (a block laid out behind the function that jumps back up is no loop)
        if ts:
            loops[h] = (ts, body & fwd)
    return loops


def loop_paths(blocks, succ, head, tails, body):
    """The way from the head to a branch back to it that issues the FEWEST vector instructions (an inner loop counts as one trip):
    its classes and its blocks."""
    counts = {i: count_block(blocks[i][1]) for i in body}
    memo, stack = {}, set()

    def walk(i):
        if i in memo:
            return memo[i]
        stack.add(i)
        opts = [walk(j) for j in succ[i] if j in body and j != head and j not in stack]
        opts = [o for o in opts if o is not None]
        stack.discard(i)
        if i in tails:
            opts.append((dict.fromkeys(CLASSES, 0), frozenset()))
        if not opts:
            return None                                   # a dead end inside an inner loop's cycle: not a way to the back edge
        lo = min(opts, key=lambda o: o[0]['VALU'])
        memo[i] = (add(counts[i], lo[0]), lo[1] | {i})
        return memo[i]

    return walk(head)


def report(text, show_all=False, out=sys.stdout):
    funcs = parse_functions(text)
    meta = kernel_metadata(text)
    names = sorted(n for n in funcs if 'render_forward_kernel' in n)
    pretty = demangle(names)
    hdr = f"{'loop':28s}" + ''.join(f'{k:>9s}' for k in CLASSES)
    for name, nice in zip(names, pretty):
        body, res = funcs[name]
        kv = meta.get(name, {})
        nice = re.sub(r'^void ', '', nice).split('(')[0]
        print(f'== {nice}', file=out)
        print(f"   VGPRs {res.get('NumVgprs', kv.get('vgpr_count', '?'))}  AGPRs {res.get('NumAgprs', kv.get('agpr_count', '?'))}"
              f"  SGPRs {res.get('NumSgprs', kv.get('sgpr_count', '?'))}  scratch {res.get('ScratchSize', kv.get('private_segment_fixed_size', '?'))} B"
              f"  VGPR spills {kv.get('vgpr_spill_count', '?')}  SGPR spills {kv.get('sgpr_spill_count', '?')}  occupancy {res.get('Occupancy', '?')}", file=out)
        blocks, index = blocks_of(body)
        print('   ' + hdr, file=out)
        succ = successors(blocks, index)
        loops = loops_of(blocks, index, succ)
        for head in sorted(loops):
            tails, body = loops[head]
            every = dict.fromkeys(CLASSES, 0)
            for i in body:
                every = add(every, count_block(blocks[i][1]))
            holds_loop = any(h2 != head and h2 in body for h2 in loops)
            if not show_all and (every['MFMA'] == 0 or holds_loop):   # by default the innermost loops with MFMAs: one trip = one wave-step of 32 samples
                continue
            lo, on_path = loop_paths(blocks, succ, head, tails, body)
            tag = f'{blocks[head][0]}{" (outer)" if holds_loop else ""}'
            print(f"   {tag + ' every block':28s}" + ''.join(f'{every[c]:9d}' for c in CLASSES), file=out)
            print(f"   {'  fewest-VALU way through':28s}" + ''.join(f'{lo[c]:9d}' for c in CLASSES), file=out)
            for i in sorted(body - on_path):                          # what that way branches over, block by block (small ones left out)
                c = count_block(blocks[i][1])
                if c['VALU'] >= 16:
                    print(f"   {'  not on it: ' + (blocks[i][0] or 'after ' + str(next(blocks[q][0] for q in range(i, -1, -1) if blocks[q][0]))):28s}"
                          + ''.join(f'{c[k]:9d}' for k in CLASSES), file=out)
        print(file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--all', action='store_true', help='list the loops without MFMAs too (phase B, prologue)')
    ap.add_argument('--keep-asm', metavar='PATH', help='write the assembly here instead of a temporary file')
    ap.add_argument('--asm', metavar='PATH', help='count an existing assembly file instead of compiling')
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = args.keep_asm or os.path.join(tmp, 'render.s')
            compile_asm(path)
            text = open(path).read()
    report(text, show_all=args.all)


if __name__ == '__main__':
    main()
