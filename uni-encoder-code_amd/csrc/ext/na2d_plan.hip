// Host-only report of the neighbourhood-attention planner (csrc/na2d_mfma.hip), so that a test which restates the planner fails
// loudly when the heuristic is retuned -- what uenc_window_attn_bwd_groups is to the window-attention backward.
// No arithmetic lives here: the tile count per workgroup is na2d_mfma_plan's, the function both launchers plan by, and the route is
// na2d_mfma_supported, the predicate uenc_na2d_fwd / uenc_na2d_bwd route by.
#include "../common.h"
#include "../na2d.h"
#include "../../../include/uenc_ext.h"

extern "C" int uenc_na2d_tiles_per_group(int B, int H, int W, int nH, int K, int dilation) {
    Na2d p = {};
    p.B = B; p.H = H; p.W = W; p.nH = nH; p.d = dilation;
    const int rc = na2d_check(p, K);
    if (rc != UENC_OK) return rc;
    if (!na2d_mfma_supported(H, W, nH, K)) return 0;
    return na2d_mfma_plan(B, H, W, nH, dilation).nt;
}
