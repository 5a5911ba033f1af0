"""Eager vs HIP-graph timing of the evaluation step (vlgae_amd/eval_step.py), beside the training step on the same box.
    python tools/time_eval_step.py                    # {viterbi, mbr} x {metrics on, off} at B = 256 / L = 40 / R = 36 object-only and B = 64 shipped
                                                      # layout; the training step at both; the host-bound path the metric kernels replace
    python tools/time_eval_step.py --one B L R [--shipped] [--mbr] [--no-metrics] [--steps=N]   # N eager steps of one configuration (for a
                                                      # rocprofv3 --kernel-trace run: tools/prof_eval_step.sh)
    python tools/time_eval_step.py --count DIR        # launches per step out of that trace (a step starts at its batch_prepare_kernel), and
                                                      # the time of the metric launches"""
import sys, time
sys.path.insert(0, '.'); sys.path.insert(0, 'tools'); sys.path.insert(0, 'tests')


def count(d):
    import csv, glob, os
    f = max(glob.glob(d + '/**/*kernel_trace.csv', recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
    starts = [i for i, r in enumerate(rows) if 'batch_prepare_kernel' in r['Kernel_Name']]
    seq = rows[starts[-2]:starts[-1]]
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    ev = [r for r in seq if 'eval_sentence_kernel' in r['Kernel_Name'] or 'eval_reduce_kernel' in r['Kernel_Name']]
    dep = [r for r in seq if 'deptree_kernel' in r['Kernel_Name']]
    print(f'{len(seq)} launches per step, kernel time {sum(map(us, seq)):.0f} us; metric launches {len(ev)} = {sum(map(us, ev)):.1f} us; '
          f'DepTree launches {len(dep)} = {sum(map(us, dep)):.1f} us')


if '--count' in sys.argv:
    count(sys.argv[sys.argv.index('--count') + 1])
    sys.exit(0)

import numpy as np, torch
from vlgae_amd import align, eval_step, train_step
dev = torch.device('cuda:0')
SHIPPED = ('rel', 'attr', 'img')


def gold_side(B, L, R, lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    wmask = torch.arange(L)[None] < lengths.cpu()[:, None]
    xy, wh = torch.rand(B, R, 2, generator=g) * 0.6, torch.rand(B, R, 2, generator=g) * 0.2 + 0.2
    vis_box = torch.cat([xy, xy + wh], -1)
    pick = torch.randint(0, R, (B, L, 2), generator=g)
    sg_box = (vis_box[torch.arange(B)[:, None, None], pick] + (torch.rand(B, L, 2, 4, generator=g) - 0.5) * 0.06).reshape(B, L, 8)
    sg_type = torch.randint(0, 4, (B, L), generator=g) * wmask
    return {k: t.to(dev) for k, t in dict(arc=torch.randint(0, L + 1, (B, L), generator=g) * wmask, vis_box=vis_box, sg_box=sg_box, sg_type=sg_type,
                                          sg_mask=sg_type != 0).items()}


def wall(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e3


def graph_of(step):
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3): step()
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(gr):
        step()
    for _ in range(5): gr.replay()
    return gr


def build_eval(B, L, R, factors, mbr, metrics, train=None):
    """An evaluation step on a training step's parameters and batch (or on a synthetic one of its own), with a synthetic gold side."""
    src = train if train is not None else eval_step.build(B, L, R, dev, factors=factors, metrics=False)
    b = src.batch
    given = dict(src.P, lengths=src.lengths, token=b['token'], tag=b['tag'], box_mask=b['box_mask'])
    if metrics:
        given.update(gold_side(B, L, R, src.lengths))
    return eval_step.build(B, L, R, dev, factors=factors, mbr_decoding=mbr, metrics=metrics, given=given)


if '--one' in sys.argv:
    i = sys.argv.index('--one')
    B, L, R = (int(a) for a in sys.argv[i + 1:i + 4])
    n = int(([a.split('=')[1] for a in sys.argv if a.startswith('--steps=')] or ['10'])[0])
    step = build_eval(B, L, R, SHIPPED if '--shipped' in sys.argv else (), '--mbr' in sys.argv, '--no-metrics' not in sys.argv)
    for _ in range(n): step()
    torch.cuda.synchronize()
    print('eager: %.3f ms/step' % wall(step, n))
    sys.exit(0)

with torch.autograd.set_multithreading_enabled(False):
    for B, L, R, factors in ((256, 40, 36, ()), (64, 40, 36, SHIPPED)):
        tag = f'B={B} L={L} R={R} {"shipped layout" if factors else "object-only"}'
        train = train_step.build(B, L, R, dev, factors=factors)
        for _ in range(5): train()
        print(f'{tag}: training step  eager {wall(train, 30):.3f} ms, graph {wall(graph_of(train).replay, 50):.3f} ms')
        for mbr in (False, True):
            for metrics in (True, False):
                step = build_eval(B, L, R, factors, mbr, metrics, train)
                for _ in range(5): step()
                eager = wall(step, 30)
                print(f'{tag}: eval step {"mbr    " if mbr else "viterbi"} metrics {"on " if metrics else "off"}  eager {eager:.3f} ms, '
                      f'graph {wall(graph_of(step).replay, 50):.3f} ms')
        # what the metric launches replace: the host half of decode_grounding_on_factor (the .tolist() of the top-5 columns and the nested
        # lists, align.grounding_lists) plus a walk over those lists per token (the numpy restatement of the counters, tests/eval_restatement.py)
        from eval_restatement import eval_counts
        step = build_eval(B, L, R, factors, False, True, train)
        out = step()
        torch.cuda.synchronize()
        bt = step.batch
        t0 = time.perf_counter()
        lists = align.grounding_lists(out['top5'], out['factor2img'], step.last['txt_mask'], bt['factor_names'], bt['vis_split'])
        t1 = time.perf_counter()
        mask = (torch.arange(L, device=dev)[None] < step.lengths[:, None]).cpu().numpy()
        eval_counts(out['arc'].cpu().numpy(), bt['arc'].cpu().numpy(), mask, step.lengths.cpu().numpy(), out['factor2img'].cpu().numpy(),
                    out['top5'].cpu().numpy(), bt['vis_box'].cpu().numpy(), bt['sg_box'].cpu().numpy(), bt['sg_type'].cpu().numpy(),
                    bt['sg_mask'].cpu().numpy(), factors)
        t2 = time.perf_counter()
        print(f'{tag}: host path  lists {1e3 * (t1 - t0):.1f} ms + per-token metric walk {1e3 * (t2 - t1):.1f} ms = {1e3 * (t2 - t0):.1f} ms per batch '
              f'({sum(len(s) for s in lists["txt_to_factor"])} query rows)')
