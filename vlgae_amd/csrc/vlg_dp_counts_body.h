// vlg_dp_counts_body.h -- the count write-out of the general, overlay and long DMV1o images, as a TEXT FRAGMENT: statements, not
// declarations.  vlg_dp_core.h includes it twice: inside dmv_run, where these statements have always stood (as the same tokens in
// the same place they compile to the same gfx950 code as before; as a function called from there they did not -- the other images'
// kernels moved by an instruction or two), and inside dmv_counts_out, which exists so that the host test of the short image's
// write-out (tests/emu/stage_short.cpp) can run THIS code on the same adjoint charts.
// In scope where it is included: SR, c (DmvCtx), io, tid, nt, x, Ne = c.Ne, P = c.P, oo = (0, 0).
    io.clear_heads(tid, nt);
    x.sync();
    const int E = io.out_extent(Ne);
    const float inv_e = 1.0f / (float)E;
    for (int idx = tid; idx < E * E; idx += nt) {
        const int h = (int)(((float)idx + 0.5f) * inv_e), ch = idx - h * E;
        float2 g = oo;
        if (h < Ne && ch < Ne) {
            if (ch < h) g = c.gI[h * P + ch];
            else if (ch > h) g = c.gI[h * P + ch + 1];
        }
        io.st_attach(h, ch, g);
    }
    if (io.wants_dec()) {
        // STOP counts: the adjoint of the width-0 span (one cell each)
        for (int idx = tid; idx < E * 4; idx += nt) {
            const int h = idx >> 2, dir = (idx >> 1) & 1, v = idx & 1;
            float g = 0.f;
            if (h < Ne) {
                const int q = h * P + h + dir;
                g = SR == VLG_SR_MAX ? c.gdecs[h * 4 + dir * 2 + v] : (v == 1 ? c.gCc[q] : 0.f) + reinterpret_cast<const float*>(c.gCi + q)[v];
            }
            io.st_dec(h, (dir * 2 + v) * 2 + 1, g);
        }
        // GO counts: dec[h,dir,v,GO] enters every incomplete span headed by h towards dir (dmv.py:36-37), so its count is a sum
        // over a row of the finished gI chart.  Four lanes per (h, dir) take every fourth cell (both valences at once) and meet in
        // a two-step butterfly: a fixed summation tree, ~10 dependent LDS reads instead of the 40 of one lane per sum (this loop was
        // 2.2 us of the 77 us launch as a serial walk).
        constexpr int GL = 4;
        for (int base = 0; base < E * 2; base += nt / GL) {
            const int grp = base + tid / GL, rr = tid % GL;
            const int h = grp >> 1, dir = grp & 1;
            float sum[2] = {0.f, 0.f};
            if (grp < E * 2 && h < Ne) {
                const float2* row = c.gI + h * P + (dir == 0 ? 0 : h + 2);      // cells (h, ch) for ch < h  |  (h, ch + 1) for ch > h
                const int n = dir == 0 ? h : Ne - 1 - h;
                for (int k = rr; k < n; k += GL) { sum[0] += row[k].x; sum[1] += row[k].y; }
            }
            x.template allreduce_sum<2>(sum, GL);
            if (grp < E * 2 && rr == 0) {
                io.st_dec(h, (dir * 2 + 0) * 2, sum[0]);
                io.st_dec(h, (dir * 2 + 1) * 2, sum[1]);
            }
        }
    }
