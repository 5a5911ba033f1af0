"""The dual-number DMV1o pass (vlg_dmv1o_expect) beside the two launches it doubles -- vlg_dmv1o_inside and
vlg_dmv1o_inside_outside (Log semiring) -- at the same shapes, each as a replayed one-launch HIP graph.
    python tools/time_dmv_expect.py [--out FILE] [--replays=N] [--repeats=R] [--yardsticks]

  shapes    B = 256, N = 41, lengths 10 ... 40;  B = 256, N = 81, lengths 20 ... 80;  B = 4, N = 200, lengths 50 ... 199     bf16 potentials
  expect    forward only (logZ, ev) and with mu + hv, direction = the potentials themselves (the entropy's launch)
  inside / inside_outside    the yardsticks
Timed with HIP events over windows of N replays, the graphs taking turns, R times; reported are the median and the spread of the
windows.  --yardsticks: only inside and inside_outside -- for a run against another build of the library (VLGAE_AMD_LIB), e.g. the
parent commit's, in the same session.  A machine without a GPU fails here: nothing is estimated."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from vlgae_amd import _C
from vlgae_amd.torch_struct import DMV1o, functional as F

dev = torch.device('cuda:0')
arg = lambda name, default: int(([a.split('=')[1] for a in sys.argv if a.startswith(f'--{name}=')] or [default])[0])
REPLAYS, REPEATS = arg('replays', 500), arg('repeats', 7)
SHAPES = ((256, 41, 10), (256, 81, 20), (4, 200, 50))     # (B, N, shortest sentence)


def batch(B, N, lo, seed=3):
    g = torch.Generator().manual_seed(seed)
    L = N - 1
    dec, attach, root = torch.randn(B, L, 2, 2, 2, generator=g), torch.randn(B, L, L, 2, generator=g), torch.randn(B, L, generator=g)
    md, ma = DMV1o.merge(dec.to(dev), attach.to(dev), root.to(dev))
    lengths = (lo + (torch.arange(B) * 7) % (N - lo)).to(dev)
    lengths[0] = N - 1
    return md.to(torch.bfloat16), ma.to(torch.bfloat16), lengths


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3): fn()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fn()
    for _ in range(10): gr.replay()
    return gr


def window(gr, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): gr.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3     # us per replay


def main():
    yardsticks_only = '--yardsticks' in sys.argv
    fns = {}
    for B, N, lo in SHAPES:
        md, ma, lengths = batch(B, N, lo)
        tag = f'B{B}_N{N}'
        fns[f'inside_{tag}'] = lambda md=md, ma=ma, lengths=lengths: F.dmv1o_run(md, ma, lengths, _C.SEMIRING_LOG, False)
        fns[f'inside_outside_{tag}'] = lambda md=md, ma=ma, lengths=lengths: F.dmv1o_run(md, ma, lengths, _C.SEMIRING_LOG, True)
        if not yardsticks_only:
            fns[f'expect_{tag}'] = lambda md=md, ma=ma, lengths=lengths: F.dmv1o_expect(md, ma, lengths, v=(md, ma))
            fns[f'expect_grad_{tag}'] = lambda md=md, ma=ma, lengths=lengths: F.dmv1o_expect(md, ma, lengths, v=(md, ma), want_mu=True, want_hv=True)
    graphs = {k: graph_of(fn) for k, fn in fns.items()}
    times = {k: [] for k in graphs}
    for _ in range(REPEATS):
        for k, gr in graphs.items():
            times[k].append(window(gr, REPLAYS))
    rec = dict(tool='time_dmv_expect', library=os.environ.get('VLGAE_AMD_LIB', 'this tree'), dtype='bf16', replays=REPLAYS, repeats=REPEATS,
               us={k: round(statistics.median(t), 2) for k, t in times.items()},
               spread_us={k: round(max(t) - min(t), 2) for k, t in times.items()})
    if not yardsticks_only:
        rec['ratio'] = {}
        for B, N, lo in SHAPES:
            tag = f'B{B}_N{N}'
            rec['ratio'][f'expect/inside_{tag}'] = round(rec['us'][f'expect_{tag}'] / rec['us'][f'inside_{tag}'], 2)
            rec['ratio'][f'expect_grad/inside_outside_{tag}'] = round(rec['us'][f'expect_grad_{tag}'] / rec['us'][f'inside_outside_{tag}'], 2)
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'a') as f:
            f.write(line + '\n')


main()
