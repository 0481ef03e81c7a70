// The MSM stage launchers of zkt_internal.h, by group: every zkt_msm.hip object (one per group) exports one table of its launchers, and these pick the table.
// An id that names no group goes to a table whose launchers reject it.
#include "msm_ws.h"

namespace zkt {

static const MsmLaunchers& launchers_of(int grp) { return grp == G_G1 ? msm_launchers_g1 : grp == G_SECP ? msm_launchers_secp : msm_launchers_g2; }
hipError_t launch_msm_to_kernel_layout(int grp, const uint32_t* abi, uint32_t* mont, uint8_t* inf, size_t n, hipStream_t s) { return launchers_of(grp).to_kernel_layout(grp, abi, mont, inf, n, s); }
hipError_t launch_msm_precompute(int grp, uint32_t* table, uint8_t* inf, size_t n, int c, int nwin, uint32_t* tmp, hipStream_t s) { return launchers_of(grp).precompute(grp, table, inf, n, c, nwin, tmp, s); }
hipError_t launch_msm_sort(const MsmPlan& P, const uint8_t* inf, const uint32_t* scalars, void* workspace, hipStream_t s) { return launchers_of(P.grp).sort(P, inf, scalars, workspace, s); }
hipError_t launch_msm_sort_batch(const MsmPlan& P, const uint8_t* inf, const uint32_t* scalars, size_t vec_stride, void* workspace, hipStream_t s) {
  return launchers_of(P.grp).sort_batch(P, inf, scalars, vec_stride, workspace, s);
}
hipError_t launch_msm_accumulate(const MsmPlan& P, const uint32_t* table, void* workspace, hipStream_t s) { return launchers_of(P.grp).accumulate(P, table, workspace, s); }
hipError_t launch_msm_reduce(const MsmPlan& P, void* workspace, uint32_t* jac, uint32_t* out_abi, hipStream_t s) { return launchers_of(P.grp).reduce(P, workspace, jac, out_abi, s); }
hipError_t launch_msm_jac_add(int grp, const uint32_t* a, const uint32_t* b, uint32_t* out, hipStream_t s) { return launchers_of(grp).jac_add(grp, a, b, out, s); }
hipError_t launch_msm_jac_sum_to_affine(int grp, const uint32_t* parts, size_t count, size_t stride, uint32_t* out_abi, hipStream_t s) {
  return launchers_of(grp).jac_sum_to_affine(grp, parts, count, stride, out_abi, s);
}

}  // namespace zkt
