// vlg_expect_kernels.h -- launch frame of the two dual-number kernels (vlg_expect.hip: DepTree, vlg_dmv_expect.hip: DMV1o), around the
// bodies of vlg_dp_expect.h / vlg_dmv_expect.h: the kernel-image dispatch and the entry points' checks in front of it.  Each .hip keeps its
// __global__ kernel and the lambda that launches it.  (The not-a-sentence block stands in each kernel: as a shared function over a
// list of (output, element count) it moved the SGPR counts and spills of every inside-outside image,
// profiles/expect_frame_neutrality.md.)
#pragma once
#include <type_traits>

#include "vlg_dp_kernels.h"
#include "vlg_dp_expect.h"

namespace vlg {

// go(GRAD, MODE, In, VIn) for the pass, the placement of the plan and the two storage types
template <int V>
using ExpectConst = std::integral_constant<int, V>;

template <bool GRAD, typename In, typename VIn, typename Go>
static int expect_mode(int mode, const Go& go) {
    using G = std::integral_constant<bool, GRAD>;
    switch (mode) {
        case 0: return go(G{}, ExpectConst<0>{}, In{}, VIn{});
        case 1: return go(G{}, ExpectConst<1>{}, In{}, VIn{});
        case 2: return go(G{}, ExpectConst<2>{}, In{}, VIn{});
        default: return go(G{}, ExpectConst<GRAD ? 3 : 2>{}, In{}, VIn{});   // (forward only: placements 2 and 3 are the same, staging only)
    }
}

template <typename In, typename VIn, typename Go>
static int expect_types(bool grad, int mode, const Go& go) {
    return grad ? expect_mode<true, In, VIn>(mode, go) : expect_mode<false, In, VIn>(mode, go);
}

template <typename Go>
static int expect_dispatch(bool grad, const DpPlan& p, int in_dtype, int v_dtype, const Go& go) {
    const int mode = placement_of(p.image);
    if (in_dtype == VLG_F32) return v_dtype == VLG_F32 ? expect_types<F32In, F32In>(grad, mode, go) : expect_types<F32In, BF16In>(grad, mode, go);
    return v_dtype == VLG_F32 ? expect_types<BF16In, F32In>(grad, mode, go) : expect_types<BF16In, BF16In>(grad, mode, go);
}

// The entry point vlg_<op> behind its arguments: the checks in the order its callers see them, the plan, and go(p, GRAD, MODE, In, VIn)
// for the image to launch.  An empty batch returns 0 here, behind the shape and the types and before any pointer is looked at.
// `required`: the names of the entry's required pointers; `buffers`: they are all set.
template <typename Layout, typename Go>
static int expect_entry(const char* op, int B, int N, int in_dtype, int v_dtype, const char* required, bool buffers, bool grad,
                        const void* ws, size_t ws_bytes, const Go& go) {
    if (int e = check_dp_args(op, B, N, in_dtype, VLG_SR_LOG)) return e;
    if (v_dtype != VLG_F32 && v_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "%s: v_dtype %d", op, v_dtype);
    if (B == 0) return 0;
    if (!buffers) return set_error(VLG_ERR_ARG, "%s: null buffer (%s are required)", op, required);
    const DpPlan p = dp_plan<Layout>(N, grad, false);
    if (int e = check_dp_workspace(op, N, p, B, ws, ws_bytes)) return e;
    return expect_dispatch(grad, p, in_dtype, v_dtype, [&](auto G, auto M, auto I, auto V) { return go(p, G, M, I, V); });
}

}  // namespace vlg
