"""VERDICT round 3 item 6, second source: the v_mad_u64_u32 instructions hipcc emits for the sweep loops of the headline kernel, times
their trip counts, must agree (0.5 %) with the per-square / per-product constants of bench.py's closed form — which
tests/test_bench_contract.py holds against the emulator's exact count.  Cross-compiles one translation unit for gfx950 (no GPU)."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc (cross-compile only)")
def test_static_tally_of_the_sweep_loops_agrees_with_the_closed_form(tmp_path):
    # the assembly goes to a file of fixed name in the temporary directory: this test's own, not one another user may hold
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "static_mad_tally.py")], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert res.returncode == 0, res.stdout + res.stderr
    out = res.stdout
    # round 5: a square's first word takes the symmetric half of X0*X0 — 10 of 18 limbs per lane and row: 1152 multiply-adds per trip
    assert "= square ((3 + 10/18) H^2 = 18432)" in out and "= product (5 H^2 = 25920)" in out
    assert "static tally agrees with (3 + 10/18) H^2 per square and 5 H^2 per product within 0.5 %: yes" in out
    # ... and the emulator's total is the closed form (within a rounding of the entry/exit terms): ~8922 H^2 per 2048-bit encryption (9833 before)
    import re
    totals = [float(x) for x in re.findall(r"= ([0-9.]+) H\^2$", out, re.M)]
    assert len(totals) == 2 and abs(totals[0] / totals[1] - 1) < 0.002 and 8900 < totals[0] < 8950, out
