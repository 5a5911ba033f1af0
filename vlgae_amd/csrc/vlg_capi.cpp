// vlg_capi.cpp -- thread-local error state and version of the C ABI (include/vlgae_amd.h).
#include "vlg_common.h"

namespace vlg {
char* error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}
}  // namespace vlg

extern "C" {
const char* vlg_last_error(void) { return vlg::error_buffer(); }
int vlg_version(void) { return 145; }   // 145: + vlg_step_batch_prepare, vlg_grounding_loss_ntok; since then only new symbols (vlg_deptree_sample, vlg_deptree_sample_blocks, vlg_deptree_expect, vlg_dmv1o_kbest, vlg_dmv1o_kbest_workspace, vlg_dmv1o_tree_counts, vlg_label_fold, vlg_label_expand, vlg_label_draw, vlg_label_lanes), no argument list changed: the number stays, a library without them fails to bind; round 6: vlg_ff_linear_act_backward takes k (256 / 512 / 32) and w_kn, + vlg_ff_linear_mlp_act_backward, vlg_ff_linear_kn, vlg_ff_transpose256 over a pointer array; 143: + vlg_ff_linear_act / _backward (fused row-streaming Linear + element-wise pass); 142: vlg_attn_fuse key_chunk + workspace + grad_dtype
}
