"""bench.py's two modes: a plain run carries the headline figure alone, `--full` everything else next to it; the timed step
is the same in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the records only --full fills (null in a plain run)
MOVED = ("fixed_input", "steady_state", "cpu_baseline")


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_an_option_and_off_by_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert a.full is False and a.no_full is False and (a.gpus, a.steps, a.warmup) == (1, 4, 2)
    a = _parse(monkeypatch, ["--full"])
    assert a.full is True and a.no_full is False
    a = _parse(monkeypatch, ["--full", "--no-full", "--no-steady"])          # the single switches still parse next to it
    assert a.full is True and a.no_full is True and a.no_steady is True


def _run(args, tmp):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "64", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp)] + args, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    def strict(tok):                      # NaN / Infinity are not JSON: the line must parse everywhere, not in Python alone
        raise AssertionError(f"{tok} in the bench line")
    return json.loads(lines[0], parse_constant=strict), {f[:-4]: np.load(os.path.join(str(tmp), f)) for f in sorted(os.listdir(str(tmp))) if f.endswith(".npy")}


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    """One cell-sized grid (64^3): the plain line has the headline fields and null where `--full` reports; `--full` fills them;
    both lines are strict JSON.  Both time the same step from the same inputs, so what the last step returned agrees to what
    two runs of one deterministic step on one input may differ by:
    * the update of the step is O(|ds|) = 1e-3 and comes from two linear solves to rtol 1e-9 of a system whose inverse is bounded by
      1 / 0.17 (largest eigenvalue of the stable state, bench.py) -- far inside |dp| <= 1e-9 and max |du| <= 1e-9;
    * operator applications: equal up to the documented wobble of the last Arnoldi steps, +-2 per solve, two solves;
    * residuals: each is the inf-norm of one stencil evaluation, whose rounding floor is 4 eps |L1|_inf |u|_inf with
      |L1|_inf <= (1 + 12 / h^2)^2 (the bound of __graft_entry__.smoke(); h = 0.196: ~1e-10); the two runs agree to twice that."""
    (tmp_path / "plain").mkdir()
    (tmp_path / "full").mkdir()
    plain, dp = _run([], tmp_path / "plain")
    full, df = _run(["--full", "--cpu-sample", "1"], tmp_path / "full")
    for d in (plain, full):
        assert d["metric"] == "newton_krylov_corrector_steps_per_s" and d["unit"] == "steps/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f64" and d["steps"] == 2 and d["warmup"] == 1
        assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3
        assert d["roofline"] is not None and d["kernels"]
    for k in MOVED:
        assert plain[k] is None, k
        assert full[k] is not None, k
    pc, fc = plain["config"], full["config"]
    for k in ("full_corrector", "cell_corrector"):
        assert pc[k] == {"converged": None, "itnewton": None, "itlinear": None, "residuals": [], "p": None}, (k, pc[k])
    assert pc["tiled_state_residual_inf"] == [None, None]
    assert fc["full_corrector"]["converged"] is True and fc["cell_corrector"]["converged"] is True
    assert all(r is not None and r <= 1e-9 for r in fc["tiled_state_residual_inf"])
    assert full["cpu_baseline"]["value"] is not None, full["cpu_baseline"]
    assert sorted(dp) == sorted(df) == sorted(("u", "p", "residuals", "itnewton", "itlinear", "converged"))
    assert np.array_equal(dp["itnewton"], df["itnewton"]) and np.array_equal(dp["converged"], df["converged"])
    assert dp["u"].shape == df["u"].shape == (64 ** 3,)
    assert dp["residuals"].shape == df["residuals"].shape == (2,)
    h = 2 * bench.CELL_L[0] / bench.CELL[0]
    floor = 4 * np.finfo(float).eps * (1.0 + 12.0 / h ** 2) ** 2 * float(np.abs(df["u"]).max())
    d_p, d_u = abs(float(dp["p"][0]) - float(df["p"][0])), float(np.abs(dp["u"] - df["u"]).max())
    d_it, d_res = abs(int(dp["itlinear"][0]) - int(df["itlinear"][0])), float(np.abs(dp["residuals"] - df["residuals"]).max())
    print("tiled residuals", fc["tiled_state_residual_inf"], "|dp|", d_p, "max |du|", d_u, "itlinear", dp["itlinear"], df["itlinear"],
          "residuals", dp["residuals"], df["residuals"], "max |dres|", d_res, "floor", floor)
    assert d_p <= 1e-9
    assert d_u <= 1e-9
    assert d_it <= 4
    assert d_res <= 2 * floor
