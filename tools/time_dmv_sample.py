"""DMV1o tree sampling (vlg_dmv1o_sample) beside the two launches it shares its inside pass and its walk with -- vlg_dmv1o_inside (Log
semiring) and vlg_dmv1o_decode (Max semiring + back-pointer walk) -- at the same shape, each as a replayed HIP graph.
    python tools/time_dmv_sample.py [--out FILE] [--replays=N] [--repeats=R] [--yardsticks]

  sample    B = 256, N = 41, S in {1, 8, 64}; B = 4, N = 41, S = 4096      counter-based draws (DeviceRng), heads + log-probabilities
  inside    B = 256 and B = 4, N = 41                                       logZ only
  decode    B = 256 and B = 4, N = 41                                       best score + heads
bf16 root-merged potentials (the training step's storage type), sentence lengths spread over 10 ... 40 as in the headline batch.  Every
graph holds ONE kernel launch (counted with the profiler where it is available).  Timed with HIP events over windows of N replays, the
graphs taking turns, R times; reported are the median and the spread of the windows.  --yardsticks: only inside and decode -- for a run
against another build of the library (VLGAE_AMD_LIB), e.g. the parent commit's, whose figures are the yardsticks of
profiles/dmv1o_sample.json.  A machine without a GPU fails here: nothing is estimated."""
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
REPLAYS, REPEATS = arg('replays', 2000), arg('repeats', 7)
N = 41
SHAPES = ((256, 1), (256, 8), (256, 64), (4, 4096))     # (B, S)


def batch(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    L = N - 1
    dec, attach, root = torch.randn(B, L, 2, 2, 2, generator=g), torch.randn(B, L, L, 2, generator=g), torch.randn(B, L, generator=g)
    md, ma = DMV1o.merge(dec.to(dev), attach.to(dev), root.to(dev))
    lengths = (10 + (torch.arange(B) * 7) % 31).to(dev)
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
    for _ in range(20): gr.replay()
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
    fns = {}
    for B in (256, 4):
        md, ma, lengths = batch(B)
        fns[f'inside_B{B}'] = lambda md=md, ma=ma, lengths=lengths: F.dmv1o_run(md, ma, lengths, _C.SEMIRING_LOG, False)
        fns[f'decode_B{B}'] = lambda md=md, ma=ma, lengths=lengths: F.dmv1o_decode(md, ma, lengths)
    blocks = {}
    if not yardsticks_only:
        from vlgae_amd.encoders import DeviceRng
        rng = DeviceRng(1, dev)
        for B, S in SHAPES:
            md, ma, lengths = batch(B)
            fns[f'sample_B{B}_S{S}'] = lambda md=md, ma=ma, lengths=lengths, S=S: F.dmv1o_sample(md, ma, lengths, S, rng=rng)
            blocks[f'sample_B{B}_S{S}'] = _C.lib().vlg_dmv1o_sample_blocks(B, N, S)
        heads, logp, logZ = fns['sample_B256_S8']()
        ref = F.dmv1o_run(*batch(256), _C.SEMIRING_LOG, False)[0]
        assert bool(torch.isfinite(logp).all()) and int(heads.max()) < N
        same_logZ = bool(torch.equal(logZ, ref.reshape(-1)))     # the same inside pass: the same bits
    launches = {k: launches_of(fn) for k, fn in fns.items()}
    graphs = {k: graph_of(fn) for k, fn in fns.items()}
    times = {k: [] for k in graphs}
    for _ in range(REPEATS):
        for k, gr in graphs.items():
            times[k].append(window(gr, REPLAYS))
    rec = dict(tool='time_dmv_sample', library=os.environ.get('VLGAE_AMD_LIB', 'this tree'), N=N, dtype='bf16', replays=REPLAYS, repeats=REPEATS,
               us={k: round(statistics.median(t), 2) for k, t in times.items()},
               spread_us={k: round(max(t) - min(t), 2) for k, t in times.items()},
               launches_per_call=launches, blocks_per_sentence=blocks)
    if not yardsticks_only:
        rec['logZ_equals_dmv1o_inside_bitwise'] = same_logZ
        for B, S in SHAPES:
            k = f'sample_B{B}_S{S}'
            rec.setdefault('us_per_tree', {})[k] = round(rec['us'][k] / (B * S), 4)
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'a') as f:
            f.write(line + '\n')


main()
