"""The skip predicate of the persistent solve (superodom_amd/csrc/lm_endgame.h, lm_parameter_tolerance_at_proposal): when a
candidate has been proposed, it is true exactly when the next lm_feed ends the solve with termination 2 -- whatever sums that lm_feed
is given.  A stand-alone program compiles the header text the kernels compile (g++ -O2 -ffp-contract=off, the library's flags) next
to lm_solver.h, walks every script of lm_script_data.py with the host controller and, after every step that asks for an evaluation,
prints the predicate beside what lm_feed does on copies of the state fed the script's sums, zeros and NaN."""
import os
import subprocess

import numpy as np
import pytest

import lm_script_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "superodom_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include "lm_endgame.h"
using namespace soicp;
static bool read_sums(LmSums& s, int& new_solve) {
  if (std::scanf("%d", &new_solve) != 1) return false;
  double* w = reinterpret_cast<double*>(&s);
  for (size_t i = 0; i < sizeof(LmSums) / 8; ++i) { unsigned long long b; if (std::scanf("%llx", &b) != 1) return false; std::memcpy(w + i, &b, 8); }
  return true;
}
int main() {
  int n_scripts;
  if (std::scanf("%d", &n_scripts) != 1) return 2;
  for (int k = 0; k < n_scripts; ++k) {
    double x0[7]; int lm_max, n, max_outer, outer;
    for (int i = 0; i < 7; ++i) { unsigned long long b; if (std::scanf("%llx", &b) != 1) return 2; std::memcpy(x0 + i, &b, 8); }
    if (std::scanf("%d %d %d %d", &lm_max, &max_outer, &outer, &n) != 4) return 2;
    LmState S; std::memset(&S, 0, sizeof S);
    double T[7], next[7]; std::memcpy(T, x0, sizeof T);
    int running = 0, have_pred = 0, pred = 0, reg_done = 0;
    for (int e = 0; e < n; ++e) {
      LmSums s; int new_solve;
      if (!read_sums(s, new_solve)) return 2;
      if (reg_done || (!new_solve && !running)) continue;  // (the outer bookkeeping of LidarSlam.cpp:119-148, as the launches skip a pass)
      if (!new_solve && have_pred) {  // the lm_feed the predicate spoke about, three times on copies of the state
        LmSums zero, nan; std::memset(&zero, 0, sizeof zero);
        double* w = reinterpret_cast<double*>(&nan);
        for (size_t i = 0; i < sizeof(LmSums) / 8; ++i) w[i] = std::numeric_limits<double>::quiet_NaN();
        const LmSums* fed[3] = {&s, &zero, &nan};
        int ends[3];
        for (int v = 0; v < 3; ++v) { LmState C = S; double nx[7]; const int m = lm_feed(C, *fed[v], nx); ends[v] = (!m && C.termination == 2) ? 1 : 0; }
        std::printf("%d %d %d %d %d %d\n", k, e, pred, ends[0], ends[1], ends[2]);
      }
      const int more = new_solve ? lm_begin(S, T, s, lm_max, next) : lm_feed(S, s, next);
      running = more; have_pred = 0;
      if (more) {  // |x - cand|^2 by lm_after_candidate's chain, as lm_control_wave forms it before the hand-off
        double sn = 0;
        for (int i = 0; i < 7; ++i) sn = SO_FMA(S.x[i] - S.cand[i], S.x[i] - S.cand[i], sn);
        pred = lm_parameter_tolerance_at_proposal(sn, S.x_norm) ? 1 : 0; have_pred = 1;
      } else {
        std::memcpy(T, S.x, sizeof T);
        ++outer; reg_done = S.num_successful == 1 || outer >= max_outer;
      }
    }
  }
  return 0;
}
"""


def _hex(v):
    return np.float64(v).tobytes()[::-1].hex()


def _sums_words(e):
    H = np.asarray(e["H"], np.float64)
    tri = [H[i, j] for i in range(6) for j in range(i, 6)]
    return [e["cost"], e["count"], *np.asarray(e["g"], np.float64), *tri, *[float(h) for h in e["hist"]]]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("endgame")
    src, exe = d / "predicate.cpp", d / "predicate"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    scripts = lm_script_data.scripts()
    text = [str(len(scripts))]
    for s in scripts:
        text.append(" ".join(_hex(v) for v in s["x0"]))
        text.append(f"{s['lm_max']} {s['max_outer']} {s['outer_iter']} {len(s['entries'])}")
        for e in s["entries"]:
            w = _sums_words(e)
            assert len(w) == 45
            text.append(f"{int(e['new_solve'])} " + " ".join(_hex(v) for v in w))
    out = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout
    return scripts, [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]


def test_predicate_is_the_next_feeds_parameter_tolerance(lines):
    scripts, rows = lines
    assert len(rows) >= 40, len(rows)
    for k, e, pred, ends_script, ends_zero, ends_nan in rows:
        assert pred == ends_script == ends_zero == ends_nan, (scripts[k]["name"], e, pred, ends_script, ends_zero, ends_nan)


def test_both_sides_of_the_predicate_are_reached(lines):
    scripts, rows = lines
    true_in = {scripts[k]["name"] for k, _, pred, *_ in rows if pred}
    false_in = {scripts[k]["name"] for k, _, pred, *_ in rows if not pred}
    assert "parameter_before_function" in true_in, true_in
    assert len(false_in) >= 10 and "function_tolerance" in false_in, false_in
    # a step that asks for an evaluation is followed by an entry in every script: none of the predicate's answers went unchecked
    steps = 0
    for s in scripts:
        with np.errstate(all="ignore"):
            logs, _ = lm_script_data.lm_ref.run_script(s)
        steps += sum(1 for lg in logs if not lg.get("skipped") and lg["more"])
    assert steps == len(rows), (steps, len(rows))
