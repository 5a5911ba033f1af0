// vlg_dp_pair.hip -- marginals AND the Viterbi tree of one batch of potentials in a single launch (dmv1o_pair_kernel,
// vlg_dp_kernels.h): what `DependencyBoxRel.lang_feat_max_tree` asks of DMV1o every step (src/model/joint.py:251-258: the partition's
// gradient for the arc marginals, the argmax for the predicted heads) and, when the parser trains on the Viterbi tree
// (`-DMV1o(...).max.sum()`, src/model/ldndmv.py:277-281), the tree counts of the same potentials as well.
#include "vlg_dp_kernels.h"

namespace vlg {

namespace {

// both plans, Log inside-outside and Max walk, must be the everything-in-LDS placement and fit one CU TOGETHER: the two workgroups of a
// sentence run side by side.  *p: the shared image (both are placement 0 at the same N) with the larger of the two LDS sizes.
bool pair_ok(int N, DpPlan* p) {
    const DpPlan lg = dp_plan<DmvLayout>(N, true, false), mx = dp_plan<DmvLayout>(N, true, true);
    *p = lg.lds_bytes > mx.lds_bytes ? lg : mx;
    return placement_of(lg.image) == 0 && placement_of(mx.image) == 0 && 2 * p->lds_bytes <= kLdsBudget;
}

template <typename In>
int launch_pair(const void* dec, const void* attach, const int64_t* lengths, int B, int N, const DpPlan& p, float* logZ, float* gdec_log,
                float* gatt_log, float* best, float* gdec_max, float* gatt_max, int64_t* heads, hipStream_t s) {
    auto k = p.image == kModeShort ? dmv1o_pair_kernel<In, kModeShort> : dmv1o_pair_kernel<In, 0>;
    return launch("dmv1o_pair_kernel", k, dim3(B, 2), dim3(kThreads), p.lds_bytes, s, (const typename In::T*)dec, (const typename In::T*)attach, lengths, N, logZ,
                  gdec_log, gatt_log, best, gdec_max, gatt_max, (long long*)heads);
}

}  // namespace

}  // namespace vlg

extern "C" {

int vlg_dmv1o_marginals_viterbi_supported(int N) {
    vlg::DpPlan p;
    return N >= 2 && N <= 255 && vlg::pair_ok(N, &p) ? 1 : 0;
}

int vlg_dmv1o_marginals_viterbi(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, float* logZ,
                                float* grad_dec, float* grad_attach, float* best_score, float* tree_dec, float* tree_attach, int64_t* heads,
                                void* stream) {
    using namespace vlg;
    if (B < 0 || N < 2) return set_error(VLG_ERR_SHAPE, "dmv1o_marginals_viterbi: need B >= 0 and N >= 2 (got B=%d N=%d)", B, N);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "dmv1o_marginals_viterbi: in_dtype %d", in_dtype);
    DpPlan p;
    if (N > 255 || !pair_ok(N, &p))
        return set_error(VLG_ERR_SHAPE, "dmv1o_marginals_viterbi: N=%d -- the two passes do not share a CU's LDS (see vlg_dmv1o_marginals_viterbi_supported); "
                         "launch vlg_dmv1o_inside_outside and vlg_dmv1o_viterbi on two streams", N);
    if (B == 0) return 0;
    if (!dec || !attach || !lengths || !logZ || !grad_attach || !best_score || !heads)
        return set_error(VLG_ERR_ARG, "dmv1o_marginals_viterbi: null buffer");
    if (tree_dec && !tree_attach) return set_error(VLG_ERR_ARG, "dmv1o_marginals_viterbi: tree_dec needs tree_attach");
    hipStream_t s = (hipStream_t)stream;
    return in_dtype == VLG_F32 ? launch_pair<F32In>(dec, attach, lengths, B, N, p, logZ, grad_dec, grad_attach, best_score, tree_dec, tree_attach, heads, s)
                               : launch_pair<BF16In>(dec, attach, lengths, B, N, p, logZ, grad_dec, grad_attach, best_score, tree_dec, tree_attach, heads, s);
}

}  // extern "C"
