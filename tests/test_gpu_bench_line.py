"""The driver's line (`python bench.py`, N = 1) on a small grid: the plain run times exactly --steps steps of the CSR loop and carries the
headline fields only, --dump-outputs writes what those steps computed (bit for bit the oracle's), and with --full the contract fields are
there, `value` is the CSR loop, and every committed PMC constant is either tied to the binary that is running (`traffic_binary_matches: true`)
or withheld -- never a number from another build.  GPU box only; the full-size line is what the driver runs itself."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def bench_line(*args, env=None):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_line_times_exactly_the_steps_asked_for_and_dumps_what_they_computed(pkg, orc, ctx, tmp_path):
    G, K, W = 64, 7, 2
    line = bench_line("--grid", str(G), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path))
    assert line["metric"] == "cg_iters_per_sec" and line["unit"] == "iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["n_gpus"] == 1 and line["steps"] == K and line["warmup"] == W and line["value_is_contract"]
    assert line["config"]["timed_steps"] == K and line["config"]["timed_regions"] == 1
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    assert abs(line["config"]["timed_seconds"] * 1e3 / K - line["ms_per_step"]) < 1e-9 * line["ms_per_step"]
    assert not {"roofline", "step_kernels", "parity_full_history", "cpu_baseline", "gmres_config3", "contract_csr_loop"} & set(line)     # --full only
    x, r, res = (np.load(tmp_path / f"{k}.npy") for k in ("x", "r", "resnorm"))
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(G, 3)
    assert x.dtype == r.dtype == res.dtype == np.float64 and x.shape == r.shape == (n,) and res.shape == (K,)
    # steps W + 1 .. W + K of cg! with reltol = 0, the device's documented reduction tree: the oracle's bits
    xo, ho = orc.cg(orc.CSC(n, colptr, rowval, nzval, 1), pkg.fixtures.hashed_rhs(n), reltol=0.0, maxiter=W + K, mode="tree", shape=ctx.cg_shape(np.float64))
    assert ho["iters"] == W + K and np.array_equal(res, ho["resnorm"][W:W + K]) and np.array_equal(x, xo)
    assert res[-1] == line["config"]["final_residual"] and abs(np.linalg.norm(r) - res[-1]) <= 1e-10 * res[-1]


def test_line_is_contract_complete_and_counters_are_tied_to_the_loaded_binary(pkg, tmp_path):
    env = dict(os.environ, MIK_BENCH_MIN_SECONDS="0.05")
    line = bench_line("--grid", "128", "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-gmres", "--no-config5",
                      "--no-f-solvers", "--no-gmres-large", "--dump-outputs", str(tmp_path), env=env)
    assert line["metric"] == "cg_iters_per_sec" and line["unit"] == "iters/s" and line["n_gpus"] == 1 and line["dtype"] == "f64" and line["value_is_contract"]
    assert line["steps"] == 20 and line["config"]["timed_steps"] == 20 and line["contract_csr_loop"]["kernel"].startswith("k_spmv_rowgather")
    x, res = np.load(tmp_path / "x.npy"), np.load(tmp_path / "resnorm.npy")       # 128^3 rows: a seeded sample of 2^20 entries
    assert x.shape == (1 << 20,) and res.shape == (20,) and res[-1] == line["config"]["final_residual"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["kernel"].startswith("k_spmv_rowgather") and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"] and r["avg_launch_ms"] <= line["ms_per_step"]
    assert "extras" not in line and "idrs8_per_step" not in json.dumps(line)              # nothing outside the scope contract on the default line
    sha = hashlib.sha256(open(pkg._lib.LIB_PATH, "rb").read()).hexdigest()
    assert r["libmik_sha256"] == sha
    src = json.load(open(os.path.join(ROOT, r["traffic_source"])))
    same = src["_binary"]["libmik_sha256"] == sha
    assert r["traffic_binary_matches"] == same
    if same:
        assert r["traffic"] == src["k_spmv_rowgather"]["traffic_bytes_per_launch"] and "_Z16k_spmv_rowgather" in src["_binary"]["mangled"]["k_spmv_rowgather<double, true, true>"]
    else:
        assert r["traffic"] is None and "traffic_withheld" in r
    for kk in line["step_kernels"]:
        assert kk["traffic_binary_matches"] in (True, False, None) and (kk["traffic"] is None or kk["traffic_binary_matches"])
