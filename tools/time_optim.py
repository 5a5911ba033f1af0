"""The optimiser step (vlgae_amd/optim.py) beside the torch formulation a user would write without it, on the leaf set of the bf16 training
step with the shipped factor layout (train_step's parameter table at B = 256, L = 40, R = 36: 6.48 M elements), each as a replayed HIP graph.
    python tools/time_optim.py [--out FILE] [--replays N] [--repeats R]

  (a) opt.update(grads)                                   two launches: clip + Adam + decay + bf16 refresh
  (b) clip_grad_norm_(foreach=True), torch.optim.Adam(fused=True, capturable=True) on float32 masters, the exponential decay as an in-graph
      `lr.mul_(gamma)` (ExponentialLR computes on the host: a captured loop cannot call it), torch._foreach_copy_ into the bf16 leaves;
      timed twice: with the gradients already float32 where the master is ("b_f32grads": the cheaper form, the one (a) is judged against), and
      from the bf16 gradients the step returns, widened by one more _foreach_copy_ ("b")
Both start from the same values and get the same gradients.  First K = 3 eager updates of each are checked against torch in float64 on the
CPU within the bounds of tests/optim_restatement.py; then the graphs are timed in alternating windows of N replays, R times.  Prints one
JSON line (and appends it to FILE): times, the spread of the repeats, launches per update, bytes per second of (a) from 28 bytes per element
plus one more read of the gradients, and its share of the 6.29 TB/s streaming rate measured for this chip (MI355X_MICROARCH: float4 copy).
A machine without a GPU fails here: nothing is estimated."""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))     # (the oracle and the bounds are the tests')
import torch

import optim_restatement as R
from vlgae_amd import optim, step_model

dev = torch.device('cuda:0')
arg = lambda name, default: int(([a.split('=')[1] for a in sys.argv if a.startswith(f'--{name}=')] or [default])[0])
REPLAYS, REPEATS, K = arg('replays', 2000), arg('repeats', 7), 3
HYPER = dict(lr=R.LR, betas=R.BETAS, eps=R.EPS, gamma=R.GAMMA, max_norm=R.MAX_NORM)
STREAM_PEAK = 6.29e12


def leaf_set(seed=5):
    """{name: (value, gradients[K])} on the CPU in the step's storage types: bf16 everywhere but ln_w / ln_b."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape, storage, init in step_model.param_table(128, 256, 800, 32, 45, 256, 150, 16, 2048, 3):
        if name in optim.FROZEN:
            continue
        dt = torch.float32 if storage == 'float32' else torch.bfloat16
        value = step_model._draw(g, shape, init)
        grads = [(torch.randn(shape, generator=g) * 0.02).to(dt) for _ in range(K)]
        out[name] = (value.to(dt), grads)
    return out


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


def within_bounds(ref, masters, opts, what):
    try:
        R.check_against(ref, dict(p=list(masters)), opts, K, what=what)
        return True
    except AssertionError as e:
        print('bound missed:', e, file=sys.stderr)
        return False


class TorchWay:
    """(b): what a training loop does today with torch ops."""

    def __init__(self, leaves, widen):
        self.names = list(leaves)
        self.leaf = [leaves[k][0].to(dev) for k in self.names]
        self.master = [t.float().clone().requires_grad_(True) if t.dtype == torch.bfloat16 else t.requires_grad_(True) for t in self.leaf]
        self.lr = torch.tensor(HYPER['lr'], device=dev)
        self.opt = torch.optim.Adam(self.master, lr=self.lr, betas=HYPER['betas'], eps=HYPER['eps'], fused=True, capturable=True)
        self.lr = self.opt.param_groups[0]['lr']
        self.widen = widen
        self.grads = [torch.zeros_like(t if widen else m) for t, m in zip(self.leaf, self.master)]        # the static gradient buffers
        for m, g in zip(self.master, self.grads):
            m.grad = torch.zeros_like(m) if widen and g.dtype != m.dtype else g
        self.narrow = [(t, m) for t, m in zip(self.leaf, self.master) if t.dtype == torch.bfloat16]
        self.wide = [(m.grad, g) for m, g in zip(self.master, self.grads) if m.grad is not g]

    def update(self):
        with torch.no_grad():
            if self.wide:
                torch._foreach_copy_([a for a, _ in self.wide], [b for _, b in self.wide])
            torch.nn.utils.clip_grad_norm_(self.master, HYPER['max_norm'], foreach=True)
            self.opt.step()
            self.lr.mul_(HYPER['gamma'])
            torch._foreach_copy_([a for a, _ in self.narrow], [b for _, b in self.narrow])


def main():
    leaves = leaf_set()
    names = list(leaves)
    n_elem = sum(v.numel() for v, _ in leaves.values())
    grad_bytes = sum(v.numel() * v.element_size() for v, _ in leaves.values())
    # ---- (a) ----
    P = {k: leaves[k][0].to(dev) for k in names}
    opt = optim.ClippedAdam(P, **HYPER)
    static = {k: torch.zeros_like(P[k]) for k in names}
    ways = dict(b=TorchWay(leaves, widen=True), b_f32grads=TorchWay(leaves, widen=False))
    # ---- both against float64 torch on the CPU, on the same gradients ----
    for k in range(K):
        for n in names:
            static[n].copy_(leaves[n][1][k])
        opt.update(static)
        for w in ways.values():
            for g, n in zip(w.grads, names):
                g.copy_(leaves[n][1][k])
            w.update()
    opts = [opt.options[n] for n in names]
    ref = R.oracle([leaves[n][0] for n in names], [[leaves[n][1][k] for n in names] for k in range(K)], opts, torch.float64)
    within = dict(a=within_bounds(ref, opt.master.values(), opts, '(a)'), **{tag: within_bounds(ref, w.master, opts, tag) for tag, w in ways.items()})
    assert all(torch.equal(P[n], opt.master[n].to(P[n].dtype)) for n in names)
    # ---- launches per update (eager, traced once) ----
    launches = dict(a=launches_of(lambda: opt.update(static)), **{tag: launches_of(w.update) for tag, w in ways.items()})
    # ---- the graphs, in alternating windows ----
    graphs = dict(a=graph_of(lambda: opt.update(static)), **{tag: graph_of(w.update) for tag, w in ways.items()})
    times = {tag: [] for tag in graphs}
    for _ in range(REPEATS):
        for tag, gr in graphs.items():
            times[tag].append(window(gr, REPLAYS))
    med = {tag: statistics.median(t) for tag, t in times.items()}
    spread = {tag: max(t) - min(t) for tag, t in times.items()}
    # per element: p, m, v read and written (24), the gradient read twice (norm, update), the bf16 shadow written
    bytes_a = 24 * n_elem + 2 * grad_bytes + sum(2 * v.numel() for v, _ in leaves.values() if v.dtype == torch.bfloat16)
    rec = dict(tool='time_optim', tensors=len(names), elements=n_elem, replays=REPLAYS, repeats=REPEATS,
               us_per_update={k: round(v, 2) for k, v in med.items()}, spread_us={k: round(v, 2) for k, v in spread.items()},
               all_us={k: [round(x, 2) for x in v] for k, v in times.items()}, launches_per_update=launches, bytes_a=bytes_a,
               a_bytes_per_s=round(bytes_a / (med['a'] * 1e-6)), a_share_of_streaming_peak=round(bytes_a / (med['a'] * 1e-6) / STREAM_PEAK, 3),
               a_faster_than_b_f32grads_beyond_spread=bool(med['b_f32grads'] - med['a'] > max(spread['a'], spread['b_f32grads'])),
               within_bounds_of_float64_torch=within,
               finite=bool(all(math.isfinite(float(opt.master[n].abs().max())) for n in names)))
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'a') as f:
            f.write(line + '\n')
    if not all(within.values()):
        sys.exit(f'outside the bounds of the float64 oracle: {within}')


main()
