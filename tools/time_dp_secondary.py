"""The DP launches beside the headline, of the library VLGAE_AMD_LIB points at (the whole library, not a headline-only variant):
the marginals + Viterbi pair launch and the inside-only launch at B = 256, L = 40, and the fused launch at L = 80 (bf16 potentials).
Five repetitions each, microseconds per launch from device events.  profiles/r08_secondary_ab.txt: two builds, alternating."""
import sys, torch
sys.path.insert(0, '.')
import vlgae_amd.torch_struct as ts
from vlgae_amd.torch_struct import functional as F
dev = torch.device('cuda:0')
def case(B, L):
    g = torch.Generator().manual_seed(1)
    dec = torch.randn(B, L, 2, 2, 2, generator=g).log_softmax(-1).to(dev)
    attach = torch.randn(B, L, L, 2, generator=g).to(dev)
    root = torch.randn(B, L, generator=g).log_softmax(-1).to(dev)
    md, ma = ts.DMV1o.merge(dec, attach, root)
    return md.bfloat16(), ma.bfloat16(), torch.full((B,), L, dtype=torch.long, device=dev)
def t(fn, n, w):
    for _ in range(w): fn()
    torch.cuda.synchronize(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize(); return e0.elapsed_time(e1) * 1e3 / n
md, ma, ln = case(256, 40)
pair = [t(lambda: ts.DMV1o([md, ma], ln).marginals_and_heads(), 200, 20) for _ in range(5)]
inside = [t(lambda: F.dmv1o_run(md, ma, ln, 0, False), 200, 20) for _ in range(5)]
md8, ma8, ln8 = case(256, 80)
long_ = [t(lambda: F.dmv1o_run(md8, ma8, ln8, 0, True), 50, 5) for _ in range(5)]
f = lambda v: ' '.join('%.2f' % x for x in v)
print('pair_us %s | inside_us %s | L80_fused_us %s' % (f(pair), f(inside), f(long_)))
