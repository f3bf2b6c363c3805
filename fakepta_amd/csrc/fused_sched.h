// k_grid_fused's draw shapes and the schedule of its DFT waves' ring iterations, in plain C++: no HIP here.
// grid_fused.hip's ring loop asks these functions what an iteration does, and a stand-alone CPU program can include
// this file alone (tests/test_fused_sched.py walks every schedule of up to 8 groups per signal with them).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FPTA_SCHED_HD __host__ __device__
#else
#define FPTA_SCHED_HD
#endif

namespace fpta {

// Draw shapes: what each prefetched term slot (kFusedTerms = 2) of each grid signal (kFusedMaxSig = 2) holds, as a
// compile-time property of a kernel instance, so that its ring iterations issue only the loads their terms read: a
// generated term its amplitude pair (one load), a loaded term its cos and sin pairs (two), an absent one none.
// launch_grid_fused picks the shaped instance when the descriptors match; every other layout runs the fallback
// (k_grid_fused_any), which reads kinds and counts from the descriptors and loads two values for every slot.
constexpr int kFusedShapeAny = 0;      // fallback
constexpr int kFusedShapeGenLoad = 1;  // signal 0 = {generated, loaded}, signal 1 = {generated}: C2 (RN + GWB, DM)
constexpr int kFusedShapeLoad = 2;     // one signal of one loaded term: a mixed common signal (C4)
constexpr int kFusedSlotAny = -1, kFusedSlotNone = 0, kFusedSlotGen = 1, kFusedSlotLoad = 2;
FPTA_SCHED_HD constexpr int fused_shape_nsig(int shape) {  // grid signals of the shape; 0: read from the descriptors
  return shape == kFusedShapeGenLoad ? 2 : shape == kFusedShapeLoad ? 1 : 0;
}
FPTA_SCHED_HD constexpr int fused_shape_slot(int shape, int s, int i) {  // term slot i of signal s
  return shape == kFusedShapeAny       ? kFusedSlotAny
         : shape == kFusedShapeGenLoad ? (i == 0 ? kFusedSlotGen : (s == 0 && i == 1 ? kFusedSlotLoad : kFusedSlotNone))
                                       : (s == 0 && i == 0 ? kFusedSlotLoad : kFusedSlotNone);
}

// The shape that serves a layout of n_sig grid signals, signal s of n_terms[s] terms of kinds kind[s][i] (0 generated,
// 1 loaded; only the first kFusedTerms = 2 of a signal are looked at, and only when it has no more). launch_grid_fused
// runs the shaped instance of its draws when this is that instance's shape, else the fallback.
FPTA_SCHED_HD constexpr int fused_shape_match(int n_sig, const int32_t* n_terms, const int32_t (*kind)[2]) {
  return n_sig == 2 && n_terms[0] == 2 && kind[0][0] == 0 && kind[0][1] == 1 && n_terms[1] == 1 && kind[1][0] == 0
             ? kFusedShapeGenLoad
         : n_sig == 1 && n_terms[0] == 1 && kind[0][0] == 1 ? kFusedShapeLoad
                                                            : kFusedShapeAny;
}

// 4-mode k-steps of a DFT job on a grid signal of nm padded modes, per parity (0: odd k, the larger; 1: even k), and
// its groups of 16 modes (two k-steps of both parities)
FPTA_SCHED_HD constexpr int32_t fused_ksteps(int32_t nm, int par) { return (((nm + (par ? 0 : 1)) >> 1) + 3) >> 2; }
FPTA_SCHED_HD constexpr int32_t fused_groups(int32_t nm) { return (fused_ksteps(nm, 0) + 1) >> 1; }

// One build (an item's accumulators) is n_it = max ng ring iterations on every DFT wave. Iteration g
//  * runs the MFMA steps of group g for the waves whose job has one (fused_steps), reading ring slot sb + g, and
//  * draws group g + 1 of every signal that has one into slot sb + g + 1; the last iteration draws group 0 of the
//    next item for every signal instead (fused_draw_group; stored unless no item follows: fused_draws).
// A shaped instance issues a signal's draw loads and a wave's table loads only in the iterations that read them
// (fused_draw_loads, fused_steps); the fallback issues all of them in every iteration.
// The kernel's loop body ends in one unconditional ring sync, so all DFT waves of a workgroup execute the same n_it
// syncs per build (n_it depends on the group counts alone, not on a wave's job), and the ring slot parity sb advances by
// n_it per build.
FPTA_SCHED_HD constexpr int32_t fused_iterations(int32_t ng0, int32_t ng1) { return ng0 > ng1 ? ng0 : ng1; }
FPTA_SCHED_HD constexpr bool fused_steps(int32_t jng, int32_t g) { return g < jng; }
FPTA_SCHED_HD constexpr bool fused_draw_loads(int32_t ng_s, int32_t g, bool last) { return last || g + 1 < ng_s; }
FPTA_SCHED_HD constexpr bool fused_draws(int32_t ng_s, int32_t g, bool last, bool nx) { return last ? nx : g + 1 < ng_s; }
FPTA_SCHED_HD constexpr int32_t fused_draw_group(int32_t g, bool last) { return last ? 0 : g + 1; }

}  // namespace fpta

#undef FPTA_SCHED_HD
