"""The ring-iteration schedule of k_grid_fused's DFT waves and its draw-shape matcher (csrc/fused_sched.h, plain C++
shared with the kernel and its launcher), run on the CPU. The schedule is walked for every pair of group counts up to 8
(one or two grid signals) over three items: every group of every signal of every item is drawn exactly once, into the
ring slot its reader then finds it in and before that read; every job steps every group of its signal once; and a
shaped instance issues a signal's draw loads exactly where a draw reads them (but for the last item's last iteration,
whose loads nothing follows). The iteration count depends on the group counts alone, which with the loop body's one
unconditional ring sync is what gives every wave the same syncs; that sync is the kernel's and is not modelled here.
The matcher: which term patterns each shape serves and which fall to the fallback. Built with the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fakepta_amd", "csrc")

_MAIN = r"""
#include <cstdio>
#include <set>
#include <tuple>
#include "fused_sched.h"
using namespace fpta;
// grid_fused.hip's build loop for item `it` of n_items, every wave at once: wave jobs are (signal, groups of it) for
// each signal and a wave without a job (jng 0).
struct Ring {
  int item[2][2], group[2][2];  // [slot][signal]
};
static int fail(const char* what, int ng0, int ng1, int it, int g) {
  std::printf("FAIL %s ng %d %d item %d g %d\n", what, ng0, ng1, it, g);
  return 1;
}
int main() {
  long walked = 0;
  for (int ng0 = 1; ng0 <= 8; ++ng0)
    for (int ng1 = 0; ng1 <= 8; ++ng1) {
      const int n_sig = ng1 > 0 ? 2 : 1, ng[2] = {ng0, ng1}, n_items = 3;
      const int n_it = fused_iterations(ng0, ng1);
      if (n_it != (ng0 > ng1 ? ng0 : ng1)) return fail("iterations", ng0, ng1, 0, 0);
      Ring ring;
      for (auto& r : ring.item) r[0] = r[1] = -1;
      std::set<std::tuple<int, int, int>> drawn, stepped[3];  // (item, signal, group); stepped per job
      int sb = 0;
      for (int it = 0; it < n_items; ++it) {
        const bool nx = it + 1 < n_items;
        if (it == 0) {  // the first item's group 0, drawn alone
          for (int s = 0; s < n_sig; ++s) {
            ring.item[sb][s] = 0;
            ring.group[sb][s] = 0;
            drawn.insert({0, s, 0});
          }
        }
        for (int g = 0; g < n_it; ++g) {
          const bool last = g + 1 == n_it;
          // steps of every job: signal js from slot sb + g; job 2 = no job
          for (int job = 0; job < 3; ++job) {
            const int js = job < n_sig ? job : -1, jng = js < 0 ? 0 : ng[js];
            if (!fused_steps(jng, g)) continue;
            const int slot = (sb + g) & 1;
            if (ring.item[slot][js] != it || ring.group[slot][js] != g) return fail("step reads", ng0, ng1, it, g);
            if (!stepped[job].insert({it, js, g}).second) return fail("step twice", ng0, ng1, it, g);
          }
          for (int s = 0; s < n_sig; ++s) {
            const bool loads = fused_draw_loads(ng[s], g, last), draws = fused_draws(ng[s], g, last, nx);
            if (draws && !loads) return fail("draw without loads", ng0, ng1, it, g);
            if (loads && !draws && !(last && !nx)) return fail("unused loads", ng0, ng1, it, g);
            if (!draws) continue;
            const int slot = (sb + g + 1) & 1, di = last ? it + 1 : it, dg = fused_draw_group(g, last);
            if (dg < 0 || dg >= ng[s]) return fail("draw group", ng0, ng1, it, g);
            // the slot's previous group of this signal has been read by now (or the signal has no job step for it)
            if (ring.item[slot][s] == it && ring.group[slot][s] >= g) return fail("draw overwrites", ng0, ng1, it, g);
            if (!drawn.insert({di, s, dg}).second) return fail("draw twice", ng0, ng1, it, g);
            ring.item[slot][s] = di;
            ring.group[slot][s] = dg;
          }
          ++walked;
        }
        sb = (sb + n_it) & 1;
      }
      for (int it = 0; it < n_items; ++it)
        for (int s = 0; s < n_sig; ++s)
          for (int g = 0; g < ng[s]; ++g) {
            if (!drawn.count({it, s, g})) return fail("never drawn", ng0, ng1, it, g);
            if (!stepped[s].count({it, s, g})) return fail("never stepped", ng0, ng1, it, g);
          }
      if ((int)drawn.size() != n_items * (ng0 + ng1)) return fail("drawn count", ng0, ng1, 0, 0);
    }
  // shapes: the slots of each, and group counts of the mode counts the tests use
  const int want[3][2][2] = {{{-1, -1}, {-1, -1}}, {{1, 2}, {1, 0}}, {{2, 0}, {0, 0}}};
  for (int sh = 0; sh < 3; ++sh)
    for (int s = 0; s < 2; ++s)
      for (int i = 0; i < 2; ++i)
        if (fused_shape_slot(sh, s, i) != want[sh][s][i]) return fail("shape slot", sh, s, i, 0);
  if (fused_shape_nsig(0) != 0 || fused_shape_nsig(1) != 2 || fused_shape_nsig(2) != 1) return fail("nsig", 0, 0, 0, 0);
  // the matcher: (signals, terms of signal 0 / 1, kinds) -> shape. 0 generated, 1 loaded.
  struct Pat {
    int n_sig;
    int32_t n_terms[2], kind[2][2];
    int want;
  };
  const Pat pats[] = {
      {2, {2, 1}, {{0, 1}, {0, 0}}, kFusedShapeGenLoad},  // C2: {generated, loaded} / {generated}
      {2, {2, 1}, {{0, 1}, {0, 1}}, kFusedShapeGenLoad},  // a kind past a signal's terms is not looked at
      {1, {1, 0}, {{1, 0}, {0, 0}}, kFusedShapeLoad},     // C4: one loaded term
      {1, {1, 1}, {{1, 1}, {1, 1}}, kFusedShapeLoad},     // (the unused second descriptor is a copy of the first)
      {2, {1, 1}, {{0, 0}, {0, 0}}, kFusedShapeAny},      // generated only
      {1, {1, 0}, {{0, 0}, {0, 0}}, kFusedShapeAny},      // one generated signal
      {2, {2, 1}, {{1, 0}, {0, 0}}, kFusedShapeAny},      // the loaded term is the anchor
      {2, {2, 1}, {{0, 1}, {1, 0}}, kFusedShapeAny},      // signal 1 loaded
      {2, {1, 1}, {{1, 0}, {1, 0}}, kFusedShapeAny},      // two loaded signals
      {2, {2, 2}, {{0, 1}, {0, 1}}, kFusedShapeAny},
      {1, {3, 0}, {{0, 0}, {0, 0}}, kFusedShapeAny},      // three coalesced members
      {1, {3, 0}, {{0, 1}, {0, 0}}, kFusedShapeAny},
      {1, {2, 0}, {{1, 0}, {0, 0}}, kFusedShapeAny},
      {2, {3, 1}, {{0, 1}, {0, 0}}, kFusedShapeAny},      // C2's pattern with a third member in signal 0
  };
  for (const Pat& p : pats)
    if (fused_shape_match(p.n_sig, p.n_terms, p.kind) != p.want)
      return fail("shape match", p.n_sig, p.n_terms[0], p.n_terms[1], p.want);
  for (int nm = 1; nm <= 400; ++nm) {  // the k-steps of both parities cover the modes, two k-steps per group
    const int q0 = fused_ksteps(nm, 0), q1 = fused_ksteps(nm, 1);
    if (4 * q0 < (nm + 1) / 2 || 4 * (q0 - 1) >= (nm + 1) / 2 || q1 > q0 || 4 * q1 < nm / 2 ||
        fused_groups(nm) != (q0 + 1) / 2)
      return fail("k-steps", nm, q0, q1, 0);
  }
  std::printf("groups %d %d %d %d %d %d\n", fused_groups(2), fused_groups(16), fused_groups(18), fused_groups(30),
              fused_groups(100), fused_groups(1));
  std::printf("ok %ld\n", walked);
  return 0;
}
"""


def test_fused_schedule_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "main.cpp").write_text(_MAIN)
    exe = str(tmp_path / "fused_sched_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "groups 1 1 2 2 7 1", lines
    # 8 x 9 pairs of group counts, three items of max(ng0, ng1) iterations each
    assert lines[1] == f"ok {3 * sum(max(a, b) for a in range(1, 9) for b in range(9))}", lines
