"""K-best DMV1o trees (vlg_dmv1o_kbest) beside vlg_deptree_kbest and the one-best launch vlg_dmv1o_decode at the same shapes, each as a
replayed HIP graph.
    python tools/time_dmv_kbest.py [--out FILE] [--replays=N] [--repeats=R] [--yardsticks]

  dmv_kbest  B = 256, N = 41, K in {1, 4, 8, 16};  B = 256, N = 81, K = 8;  B = 4, N = 200, K = 16      heads + scores + count
  dep_kbest  the same (B, N, K) on arc scores [B,N,N]                                                  heads + scores + count
  decode     vlg_dmv1o_decode at the same three (B, N)                                                 best score + heads
  counts     vlg_dmv1o_tree_counts of the K trees of the first shape's K = 16 result (the backward of kbest_scores)
bf16 potentials (the training step's storage type), sentence lengths spread over N/4 ... N - 1.  Every graph holds ONE kernel launch
(counted with the profiler where it is available).  Timed with HIP events over windows of N replays, the graphs taking turns, R times;
reported are the median and the spread of the windows, and dmv_kbest / dep_kbest and dmv_kbest / decode per shape.  --yardsticks: only
dep_kbest and decode -- for a run against another build of the library (VLGAE_AMD_LIB), e.g. the parent commit's, whose figures are the
yardsticks of profiles/dmv1o_kbest.json.  A machine without a GPU fails here: nothing is estimated."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from vlgae_amd.torch_struct import functional as F

dev = torch.device('cuda:0')
arg = lambda name, default: int(([a.split('=')[1] for a in sys.argv if a.startswith(f'--{name}=')] or [default])[0])
REPLAYS, REPEATS = arg('replays', 1000), arg('repeats', 5)
SHAPES = ((256, 41, (1, 4, 8, 16)), (256, 81, (8,)), (4, 200, (16,)))     # (B, N, Ks)


def batch(B, N, seed=3):
    g = torch.Generator().manual_seed(seed)
    dec = torch.randn(B, N, 2, 2, 2, generator=g).to(torch.bfloat16).to(dev)
    attach = torch.randn(B, N, N, 2, generator=g).to(torch.bfloat16).to(dev)
    arc = torch.randn(B, N, N, generator=g).to(torch.bfloat16).to(dev)
    lengths = (N // 4 + (torch.arange(B) * 7) % (N - N // 4)).to(dev)
    lengths[0] = N - 1
    return dec, attach, arc, lengths


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2): fn()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fn()
    for _ in range(3): gr.replay()
    return gr


def window(gr, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): gr.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3     # us per replay


def launches_of(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower())
    except Exception as e:                 # no tracer on this machine: say so instead of guessing
        return f'not measured ({type(e).__name__})'


def main():
    yardsticks_only = '--yardsticks' in sys.argv
    fns, replays = {}, {}
    for B, N, Ks in SHAPES:
        dec, attach, arc, lengths = batch(B, N)
        fns[f'decode_B{B}_N{N}'] = lambda dec=dec, attach=attach, lengths=lengths: F.dmv1o_decode(dec, attach, lengths)
        for K in Ks:
            fns[f'dep_kbest_B{B}_N{N}_K{K}'] = lambda arc=arc, lengths=lengths, K=K: F.deptree_kbest(arc, lengths, K)
            if not yardsticks_only:
                fns[f'dmv_kbest_B{B}_N{N}_K{K}'] = lambda dec=dec, attach=attach, lengths=lengths, K=K: F.dmv1o_kbest(dec, attach, lengths, K)
    if not yardsticks_only:   # what is timed is right: the ranks are sorted, all exist, rank 0 is the decode's tree
        heads, scores, count = fns['dmv_kbest_B256_N41_K16']()
        best, hd = fns['decode_B256_N41']()
        assert bool((scores[:-1] >= scores[1:]).all()) and int(count.min()) == 16 and int(heads.max()) < 41
        assert float((heads[0] == hd).float().mean()) > 0.98 and bool(((scores[0] - best).abs() <= 1e-3 * best.abs().clamp(min=1)).all())
        ln = batch(256, 41)[3]
        w = torch.ones_like(scores)
        fns['counts_B256_N41_T16'] = lambda: F.dmv1o_tree_counts(heads, ln, count, w)
    launches = {k: launches_of(fn) for k, fn in fns.items()}
    graphs = {k: graph_of(fn) for k, fn in fns.items()}
    for k, gr in graphs.items():   # a window is about a quarter of a second, whatever the launch takes
        replays[k] = max(5, min(REPLAYS, int(0.25e6 / max(window(gr, 2), 1.0))))
    times = {k: [] for k in graphs}
    for _ in range(REPEATS):
        for k, gr in graphs.items():
            times[k].append(window(gr, replays[k]))
    rec = dict(tool='time_dmv_kbest', library=os.environ.get('VLGAE_AMD_LIB', 'this tree'), dtype='bf16', replays=replays, repeats=REPEATS,
               us={k: round(statistics.median(t), 2) for k, t in times.items()},
               spread_us={k: round(max(t) - min(t), 2) for k, t in times.items()}, launches_per_call=launches)
    if not yardsticks_only:
        shapes = [(B, N, K) for B, N, Ks in SHAPES for K in Ks]
        rec['dmv_over_dep_kbest'] = {f'B{B}_N{N}_K{K}': round(rec['us'][f'dmv_kbest_B{B}_N{N}_K{K}'] / rec['us'][f'dep_kbest_B{B}_N{N}_K{K}'], 2)
                                     for B, N, K in shapes}
        rec['dmv_kbest_over_decode'] = {f'B{B}_N{N}_K{K}': round(rec['us'][f'dmv_kbest_B{B}_N{N}_K{K}'] / rec['us'][f'decode_B{B}_N{N}'], 2)
                                        for B, N, K in shapes}
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'a') as f:
            f.write(line + '\n')


main()
