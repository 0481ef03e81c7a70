// What the units of the MSM pipeline share: constants, the plan's helpers, the carve-up of a workspace and the per-group launcher tables.  zkt_msm_plan.cpp defines the
// plans and the carve, zkt_msm.hip (once per group, with msm_sort.h and msm_reduce_coop.h) the kernels and their launchers, zkt_msm_dispatch.cpp the by-group entry points.
// Everything declared here is host code; ZKT_SIDE_PRIO alone is for kernels.  The plan unit and the host check include this header for the plans and the carve and
// reference neither the macro nor the launcher tables, so they link without any zkt_msm.hip object.
#pragma once
#include "zkt_internal.h"
#include "zkt_constants.h"

// Kernels of the sort and reduce stages run beside the VALU-saturating accumulate waves of a neighbouring MSM; raise
// their wave priority so their (few, latency-bound) instructions are not queued behind them.
#ifndef ZKT_SIDE_PRIO
#define ZKT_SIDE_PRIO __builtin_amdgcn_s_setprio(3)
#endif

namespace zkt {

// Words of a coordinate IN MEMORY, which are not the limbs of its field: the G1 object may run Fq on 13 x 30-bit limbs in the 14-word slots of the 14 x 28 layout
// (zkt_msm.hip, Coord), so that every size the host code knows (table entries, bucket sums, the 42-word Jacobian partial of include/zkt.h) is the same for both.
// Affine point = 2 words of these, XYZZ = 4, Jacobian partial = 3.
constexpr int coord_words(int grp) { return grp == G_G1 ? FqC::N : grp == G_G2 ? 2 * FqC::N : SpC::N; }

// dimensions of the atomic-free partition sort (msm_sort.h, k_part_*): partitions of PART_SUB buckets, tiles of PART_TILE scalars, chunks of PART_CHUNK records
static constexpr int PART_LO = 9, PART_SUB = 1 << PART_LO, PART_TPB = 256, PART_TILE = 4 * PART_TPB, PART_CHUNK = 8192, PART_MAXP = 2048;
static constexpr int SCAN_TILE = 2048;            // counters one block of launch_scan takes; its scratch holds one word per block
static constexpr uint32_t CHUNK = 128;            // the largest chunk (MsmPlan::chunk <= CHUNK): one size bin per possible task size
static constexpr int SIZE_BINS = CHUNK + 1;       // bin k holds tasks of size CHUNK - k
// Buckets cut into more than HOT_NT pieces (a witness full of one value; the carry window of a plan whose windows end exactly at the scalars' top bit: half of
// all scalars then meet in bucket 0) are listed in hot[1..], hot[0] counting them: their partial sums are merged by HOT_FAN blocks each (k_merge_hot) instead
// of one wave walking thousands of partials.  More than HOT_CAP of them: the list is ignored and k_merge_partials does them all.
static constexpr uint32_t HOT_NT = 512, HOT_CAP = 64, HOT_FAN = 64;
static constexpr int WB_SPLIT = 4;                // blocks every bit class of k_weight_bits is cut into (msm_reduce_coop.h)

struct PartDims { uint32_t P, ntiles, maxblk; };
PartDims part_dims(size_t n, size_t nbuckets, int nwin);
size_t part_ws_bytes(size_t n, size_t nbuckets, int nwin);
uint32_t pick_chunk(size_t entries, int grp);

struct MsmWs {   // workspace carve-up (one per in-flight MSM)
  uint32_t *zero_begin, *counts, *cursor, *size_hist, *size_off, *size_cur, *hot, *zero_end;   // [zero_begin, zero_end) is cleared per MSM
  uint32_t *offsets, *entries, *slot, *sums, *colsum, *rowsum, *clsA, *clsB, *win_jac, *scan_tmp, *ntask, *task_off, *partial, *hot_part;
  uint32_t *tilehist, *tileoff, *blkoff, *subhist, *part_scan; uint2* rec;   // the partition sort; rec = (entry, low bits of the bucket id) per digit
  uint2* order; size_t max_tasks;
  uint8_t* end;                    // one past the last byte the carve hands out
};
MsmWs carve(const MsmPlan& P, void* workspace);

// The stages of one group, as its zkt_msm.hip object exports them.  The launchers of group-dependent kernels reject another group's id with hipErrorInvalidValue.
struct MsmLaunchers {
  hipError_t (*to_kernel_layout)(int grp, const uint32_t* abi, uint32_t* mont, uint8_t* inf, size_t n, hipStream_t s);
  hipError_t (*precompute)(int grp, uint32_t* table, uint8_t* inf, size_t n, int c, int nwin, uint32_t* tmp, hipStream_t s);
  hipError_t (*sort)(const MsmPlan& P, const uint8_t* inf, const uint32_t* scalars, void* workspace, hipStream_t s);
  hipError_t (*sort_batch)(const MsmPlan& P, const uint8_t* inf, const uint32_t* scalars, size_t vec_stride, void* workspace, hipStream_t s);
  hipError_t (*accumulate)(const MsmPlan& P, const uint32_t* table, void* workspace, hipStream_t s);
  hipError_t (*reduce)(const MsmPlan& P, void* workspace, uint32_t* dev_result_jac, uint32_t* dev_out_abi, hipStream_t s);
  hipError_t (*jac_add)(int grp, const uint32_t* a, const uint32_t* b, uint32_t* out, hipStream_t s);
  hipError_t (*jac_sum_to_affine)(int grp, const uint32_t* parts, size_t count, size_t stride, uint32_t* out_abi, hipStream_t s);
};
extern const MsmLaunchers msm_launchers_g1, msm_launchers_g2, msm_launchers_secp;

}  // namespace zkt
