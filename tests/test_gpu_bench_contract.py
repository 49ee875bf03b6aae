"""bench.py's output contract: exactly one JSON line on stdout with the driver's keys and the `roofline` object of the
dominant HBM-bound kernel; with --full also the `cpu_baseline` object (bounded oracle sample) and every other figure."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_contract_line(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--preroll", "8", "--full"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                     ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[key], typ), (key, d[key])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "cells/s" and d["dtype"] == "f64" and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert "merged" in d["config"]["workload"] and d["config"]["rows_per_rank"] == 1800
    assert "workload" in d["config"] and "model" not in d["config"]
    # value = cells of one step / step time
    assert abs(d["value"] - 3600 * 1800 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    zb, pb = 73440000, 4 * 1808 * 83 * 128
    r = d["roofline"]                                # the fill kernel the step launches (the product's default: one merged launch)
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and "k_fill_merged" in r["kernel"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.1 < r["frac"] < 1.0
    assert r["algorithmic_bytes_per_launch"] == zb + pb and (r["traffic"] is None or r["traffic"] >= 0.95 * (zb + pb))
    assert abs(r["launch_ms"] - d["fill_ms"]) < 1e-12 and r["launch_ms"] < d["ms_per_step"]
    f = d["roofline_fold"]                           # the fold alone (north_star's kernel), K launches in step context + copy ceiling
    assert f["bound"] == "hbm" and "k_zipper_cols" in f["kernel"] and f["algorithmic_bytes_per_launch"] == zb
    assert abs(f["frac"] - f["achieved"] / f["peak"]) < 1e-12 and 0.2 < f["frac"] < 1.0
    assert f["traffic"] is None or f["traffic"] >= 0.95 * zb
    rp = d["roofline_precompute"]                    # FP64-issue bound: that is its `bound` / `frac`; the store stream is secondary
    assert rp["bound"] == "fp64_valu" and rp["unit"] == "TFLOP/s" and rp["peak"] == 78.6 and abs(rp["frac"] - rp["achieved"] / rp["peak"]) < 1e-12
    assert 0.05 < rp["frac"] < 1.0 and 0.05 < rp["hbm_frac"] < 1.0 and rp["evaluated_cells"] == 3600 * 1800 and rp["stored_cells"] == 3608 * 1808
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["unit"] == "cells/s" and c["value"] > 1e5 and "oracle" in c["sample"]
    assert d["value"] > 100 * c["value"]            # sanity: the HIP path is the thing measured, not the oracle
    a = c["all_cores"]                               # single thread AND all cores, core count stated
    assert a["cores"] >= 1 and a["nproc"] >= a["cores"] and a["value"] > 0
    # cold and warm fold launch durations, the same-shape copy ceiling, and the same states for the merged fill
    assert 0 < d["zipper_warm_ms"] <= d["zipper_cold_dirty_ms"] * 1.5 and d["zipper_cold_ms"] > 0 and d["zipper_copy_ceiling_ms"] > 0
    assert f["copy_ceiling_ms"] == d["zipper_copy_ceiling_ms"]
    assert d["fill_merged_cold_ms"] > d["zipper_cold_ms"] and d["fill_merged_warm_ms"] > 0
    assert d["config2_quarter_degree_build"]["cells_per_s"] > 1e9
    f32 = d["float32"]                               # the reference tests both element types (test/runtests.jl:10)
    assert f32["fold_algorithmic_bytes"] == zb // 2 and 0 < f32["fold_ms"] < d["zipper_cold_ms"] * 1.2
    assert f32["fill_algorithmic_bytes"] == (zb + pb) // 2 and f32["build_cells_per_s"] > 1e9
    # what precedes the W warm-up steps is DECLARED, not implied by a missing key: the clock pre-roll with its build count (here the
    # --preroll 8 of the command line; default 64) and nothing else -- every auxiliary measurement runs after the timed region
    pre = d["clock_preroll"]
    assert pre["builds"] == 8 and pre["ms"] > 0 and "tpg_build_grid" in pre["what"] and "aux_order" not in d and "prewarm_steps" not in d
    assert f32["preroll_builds"] == 64 and "pre-roll" in f32["build_note"]
    co = d["cold_onset"]                             # the same K steps right after >= 50 ms of HBM-bound work: a caller's first builds
    assert d["ms_per_step_cold_onset"] == co["ms_per_step"] > 0 and co["steps"] == 3 and co["preceded_by_ms_of_hbm_bound_work"] >= 50
    assert 0.3 * d["ms_per_step"] < d["ms_per_step_cold_onset"] < 3 * d["ms_per_step"]
    # SURVEY 7 hard part 3: the batched-fields fold beside the 4-field headline, same geometry, one launch of 8 and of 16 fields
    fb = d["roofline_fold_batched"]
    assert [b["fields"] for b in fb] == [8, 16] and [b["algorithmic_bytes_per_launch"] for b in fb] == [2 * zb, 4 * zb]
    for b in fb:
        assert abs(b["frac"] - b["achieved"] / 8000.0) < 1e-12 and f["frac"] * 0.8 < b["frac"] < 1.0
        assert b["merged_fill_algorithmic_bytes"] == (zb + pb) * b["fields"] // 4 and 0.1 < b["merged_fill_frac"] < 1.0
    assert fb[1]["launch_ms"] > fb[0]["launch_ms"] > f["launch_ms"]
    assert "exchange_ms" not in d and "periodic_x" not in d and "line_frac_of_hbm_peak" not in json.dumps(d)
    # config 5: the fills of one baroclinic step at 1/24 degree x 100 levels
    fs = d["fill_step"]
    assert "skipped" in fs or (fs["fill3d_us"] > 0 and fs["substep_fills_us"] > 0 and fs["substeps"] == 30
                               and abs(fs["total_us"] - fs["fill3d_us"] - fs["substep_fills_us"]) < 1e-6 and fs["fields_GB"] > 160
                               and 0.5 * fs["fill3d_us"] < fs["fill3d_cold_us"] < 1.5 * fs["fill3d_us"])
    # the same fills at the reference's own model halo (5, 5, 5) (examples/bickley_jet.jl:21), halo 4 by the same method beside them:
    # ONE launch per fill at the odd Hx too (the first kernel's duration is the whole call's, minus the event bracket's overhead)
    h5 = d["fill_step_halo5"]
    a5, a4 = h5["headline_halo5"], h5["headline_halo4_same_method"]
    assert a5["halo"] == [5, 5, 5] and a4["halo"] == [4, 4, 4] and a4["fill_algorithmic_bytes"] == zb + pb
    assert a5["fill_algorithmic_bytes"] == 90720000 + 4 * 1810 * 85 * 160 and a5["fold_algorithmic_bytes"] == 90720000
    assert 0 < a5["fill_first_kernel_ms"] <= a5["fill_ms"] < a5["fill_first_kernel_ms"] + 0.03          # one launch, not two
    assert 0.7 < h5["headline_time_per_byte_halo5_over_halo4"] < 1.25 and 0.7 < h5["headline_fold_time_per_byte_halo5_over_halo4"] < 1.25
    f32 = h5["headline_float32"]                                              # Float32 rows of 3610 elements are no 16-B rows: still one launch, no slower per byte
    assert f32["halo5"]["eltype"] == "Float32" and 0.6 < f32["time_per_byte_halo5_over_halo4"] < 1.25 and 0.6 < f32["fold_time_per_byte_halo5_over_halo4"] < 1.25
    assert f32["halo5"]["fill_first_kernel_ms"] > 0.6 * f32["halo5"]["fill_ms"]
    if "skipped" not in h5.get("config5_halo5", {"skipped": 1}):
        assert h5["config5_halo5"]["fields_GB"] > 164 and 0.7 < h5["config5_time_per_byte_halo5_over_halo4"] < 1.25


FULL_ONLY = ("cpu_baseline", "roofline_fold", "roofline_precompute", "cold_onset", "ms_per_step_cold_onset", "precompute_ms", "fill_bracket_ms",
             "zipper_cold_ms", "float32", "roofline_fold_batched", "config2_quarter_degree_build", "fill_step", "fill_step_halo5")


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(gpu, oracle, tmp_path):
    """A plain run (no --full) is the headline alone: the same contract keys, nothing the --full passes measure.  --dump-outputs writes
    a fixed sample of the last timed step's outputs that does not depend on --steps / --warmup: the grid arrays as the oracle builds
    them (<= 1e-12 relative), the fields' interior as the synthetic input, their periodic-x halo as the interior it copies."""
    import numpy as np
    import bench
    from helpers import max_rel_err, splitmix64
    for steps, warmup in ((2, 1), (5, 0)):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--dump-outputs", str(tmp_path / f"s{steps}")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        out = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(out) == 1, out
        d = json.loads(out[0])
        assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1 and d["unit"] == "cells/s" and d["dtype"] == "f64"
        assert d["higher_is_better"] is True and abs(d["value"] - 3600 * 1800 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        assert d["roofline"]["launch_ms"] == d["fill_ms"] > 0 and d["clock_preroll"]["builds"] == 64
        assert not [k for k in FULL_ONLY if k in d], [k for k in FULL_ONLY if k in d]
    names = sorted(f.name for f in (tmp_path / "s2").iterdir())
    assert names == sorted(f.name for f in (tmp_path / "s5").iterdir()) and len(names) == 20 + 2 * 4
    assert sum((tmp_path / "s2" / n).stat().st_size for n in names) <= 64 << 20
    dumps = {n[:-4]: np.load(tmp_path / "s2" / n) for n in names}
    for n, a in dumps.items():                                                   # the same inputs, the same outputs, whatever K and W
        assert a.dtype == np.float64 and np.array_equal(a, np.load(tmp_path / "s5" / (n + ".npy"))), n
    g_idx, halo_idx, in_idx = bench.dump_indices()
    ref = oracle.build_grid((3600, 1800, 75))
    for name, r in ref.items():
        err, _ = max_rel_err(dumps["grid_" + name], r.reshape(-1)[g_idx])
        assert err <= 1e-12, (name, err)
    (Nx, Ny, Nz), H = (3600, 1800, 75), 4
    cols, plane = Nx + 2 * H, (Ny + 2 * H) * (Nx + 2 * H)

    def synthetic(seed, idx):                                                    # tests/helpers.synthetic_field at flat indices
        k, rem = np.divmod(idx, plane)
        j, i = np.divmod(rem, cols)
        with np.errstate(over="ignore"):
            h = splitmix64(np.uint64(seed) ^ splitmix64(idx.astype(np.uint64)))
        v = ((h >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -52 - 1.0
        inside = (k >= H) & (k < H + Nz) & (j >= H) & (j < H + Ny) & (i >= H) & (i < H + Nx)
        return np.where(inside, v, 12345.0)

    for fid, name in enumerate(("c", "u", "v", "zeta")):
        j = (in_idx % plane) // cols
        keep = j < H + Ny - 1                                                    # row Ny: the zipper's substitution for c / u
        assert np.array_equal(dumps[name + "_interior"][keep], synthetic(0x5EED + fid, in_idx[keep])), name
        k, rem = np.divmod(halo_idx, plane)
        j, i = np.divmod(rem, cols)
        west = (k >= H) & (k < H + Nz) & (j >= H) & (j < H + Ny - 1) & (i < H)
        east = (k >= H) & (k < H + Nz) & (j >= H) & (j < H + Ny - 1) & (i >= H + Nx)
        assert west.sum() > 1000 and east.sum() > 1000
        assert np.array_equal(dumps[name + "_halo"][west], synthetic(0x5EED + fid, halo_idx[west] + Nx)), name
        assert np.array_equal(dumps[name + "_halo"][east], synthetic(0x5EED + fid, halo_idx[east] - Nx)), name


def _two_rank_bench(extra, launcher="self", ranks=2):
    """two ranks on this one GPU (TPG_BENCH_REHEARSE=1: gloo, host-staged seams).  launcher "self": `python bench.py --gpus 2`, no
    launcher on the command line -- bench.py starts its own workers (what the driver's N = 1 command form becomes at N > 1);
    "torchrun": the documented `python -m torch.distributed.run ...` form."""
    env = dict(os.environ, TPG_BENCH_REHEARSE="1", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "2", "--warmup", "1"] + extra
    if launcher == "self":
        cmd = [sys.executable] + tail
    else:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + tail
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), p.stdout[-2000:]       # stdout is the one contract line, nothing else
    return json.loads(lines[0])


def test_bench_two_ranks_rehearsal(gpu):
    """The N > 1 code path of bench.py as FRESH child processes: `python bench.py --gpus 2` with NO launcher -- bench.py spawns its
    two workers itself, before importing torch -- both on this one GPU, seam messages host-staged over gloo (RCCL refuses two ranks
    on one device; the RCCL leg itself is test_bench_loopback_runs_the_rccl_branch and tests/test_gpu_exchange.py).  Default =
    STRONG scaling = BASELINE config 4's geometry (the 3600 x 1800 x 75 globe in N bands; N = 2 here: 900 rows each, the zipper on
    rank 1); `--scaling weak` is the named alternative, run here through torchrun (the other launch form).  Timings of such a run
    mean nothing; the contract does."""
    d = _two_rank_bench([])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "strong"
    assert d["config"]["global_size"] == [3600, 1800, 75] and d["config"]["local_size"] == [3600, 900, 75]
    assert d["config"]["rows_per_rank"] == 900 and d["config"]["parallelism"] == "latitude-bands x2" and "config 4" in d["config"]["workload"]
    assert isinstance(d["exchange_ms"], float) and d["exchange_ms"] > 0 and "gloo" in d["exchange_transport"]
    assert d["exchange_form"] == "monolithic" and d["exchange_ms_monolithic"] == d["exchange_ms"] and d["exchange_ms_pipelined"] is None
    assert d["pipelined_probe"]["status"] == "not run" and d["ms_per_step_by_form"] == {"monolithic": d["ms_per_step"]}    # fallback transport: one form
    assert abs(d["link_floor_ms"] - 4 * 3608 * 4 * 83 * 8 / 153.6e9 * 1e3) < 1e-9
    assert d["seam_GBps_per_direction"] > 0 and d["overlap"] is not None and 0.0 <= d["overlap_hidden_frac"] <= 1.0
    assert d["exchange_over_build"] > 0 and d["fill_plus_exchange_ms"] >= d["exchange_ms"]
    assert abs(d["value"] - 3600 * 1800 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]            # the globe is fixed: strong
    assert d["precompute_cells_per_s"] > 0 and d["roofline"]["launch_ms"] > 0
    assert d["precompute_steady_ms"] > 0 and abs(d["precompute_steady_cells_per_s"] - 3600 * 1800 / (d["precompute_steady_ms"] * 1e-3)) < 1e-3 * d["precompute_steady_cells_per_s"]
    rp = d["roofline_precompute"]
    assert rp["bound"] == "fp64_valu" and rp["unit"] == "TFLOP/s" and abs(rp["frac"] - rp["achieved"] / rp["peak"]) < 1e-12
    assert rp["evaluated_cells"] == 3600 * 904 and rp["stored_cells"] == 3608 * 908                   # a 900-row band + one seam's halo rows
    pr = d["per_rank"]                                                # every rank's own phase times
    assert [r["rank"] for r in pr] == [0, 1] and pr[0]["rows"] == [1, 900] and pr[1]["rows"] == [901, 1800]
    assert [r["zipper"] for r in pr] == [False, True] and [r["seams"] for r in pr] == [1, 1] and all(r["build_ms"] > 0 for r in pr)
    assert all(r["seams_bit_exact"] for r in pr)                      # each rank rebuilt its neighbour's field and compared the halo rows it received
    assert "cpu_baseline" not in d and "fill_step" not in d           # rank 0 at N = 1 only
    w = _two_rank_bench(["--scaling", "weak"], launcher="torchrun")
    assert w["scaling"] == "weak" and w["config"]["global_size"] == [3600, 3600, 75] and w["config"]["local_size"] == [3600, 1800, 75]
    assert abs(w["value"] - 2 * 3600 * 1800 / (w["ms_per_step"] * 1e-3)) <= 1e-6 * w["value"]


def test_bench_four_ranks_rehearsal_interior_ranks_verify_both_seams(gpu):
    """`python bench.py --gpus 4` (self-started workers, gloo rehearsal on this one GPU): the two interior ranks carry two seams each, with
    different neighbours on either side, and every rank's bit-exact seam verification must pass (each rebuilds BOTH neighbours' rows)."""
    d = _two_rank_bench([], ranks=4)              # 4 workers + this test process = 5 holders of the card; the box's process guard allows 6, and
    # the suite keeps one in reserve (a 6-rank rehearsal from inside pytest was killed at 7 holders in round 5): N = 5, 6 are run by hand
    # outside pytest (profiles/r05/rehearsal_6ranks.json), config 4's own N = 8 start-up device-free in tests/test_bench_startup.py
    assert d["n_gpus"] == 4 and d["config"]["rows_per_rank"] == 450 and d["config"]["parallelism"] == "latitude-bands x4"
    assert d["clock_preroll"]["builds"] == 64 * 4 and d["ms_per_step_cold_onset"] is None
    pr = d["per_rank"]
    assert [r["rows"] for r in pr] == [[1, 450], [451, 900], [901, 1350], [1351, 1800]]
    assert [r["seams"] for r in pr] == [1, 2, 2, 1] and [r["zipper"] for r in pr] == [False, False, False, True]
    assert all(r["seams_bit_exact"] for r in pr) and "bit for bit" in d["seam_check"]
    assert abs(d["value"] - 3600 * 1800 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]


def test_bench_production_branch_between_real_processes_over_the_test_double(gpu):
    """`TPG_BENCH_REHEARSE=shim python bench.py --gpus 4`: the branch the driver's multi-GPU run takes (`comm is not None`: RcclComm.from_torch at
    world 4, seam buffers, tpg_fill_halo_regions_distributed_peers and both pipelined forms at first contact, the pre-pass that picks a form by
    max-over-ranks time, the side / comm streams, per-form instrumented passes) -- between four real processes with different neighbours on
    either side, its librccl entry points served by the test double tools/nccl_shim behind the test library.  Until round 5 this branch had only
    ever run at world size 1 (--loopback); the gloo rehearsals above take the FALLBACK transport.  Every rank verifies its seams bit for bit."""
    env = dict(os.environ, TPG_BENCH_REHEARSE="shim", MASTER_ADDR="127.0.0.1", TPG_SHIM_DEADLINE_S="60")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TPG_RCCL_LIBRARY"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1", "--preroll", "8"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["config"]["rows_per_rank"] == 450 and "TEST DOUBLE of librccl" in d["exchange_transport"]
    forms = {"monolithic", "pipelined_1", "pipelined_2"}
    assert set(d["exchange_prepass_fill_ms"]) == forms and d["exchange_form"] in forms                 # all three forms ran on every rank
    assert d["exchange_ms_monolithic"] > 0 and d["exchange_ms_pipelined_1"] > 0 and d["exchange_ms_pipelined_2"] > 0
    pr = d["per_rank"]
    assert [r["seams"] for r in pr] == [1, 2, 2, 1] and [r["zipper"] for r in pr] == [False, False, False, True]
    assert all(r["seams_bit_exact"] for r in pr) and all(set(r["exchange_ms_by_form"]) == forms for r in pr)
    assert d["roofline"]["launch_ms"] > 0                                                              # the zipper band's merged fold ran (rank 3)
    # the run was made with the monolithic form first; the pipelined forms were probed afterwards (fresh fields, seam check, pre-pass) and passed
    assert d["pipelined_probe"] == {"status": "ok", "forms": {"pipelined_1": "ok", "pipelined_2": "ok"}}
    assert "monolithic" in d["ms_per_step_by_form"] and d["ms_per_step"] == d["ms_per_step_by_form"][d["exchange_form"]]


def test_bench_a_stalled_pipelined_probe_costs_the_probe_not_the_line(gpu):
    """The pipelined exchange forms have never met a second RCCL rank.  They are probed only AFTER the run has been made with the monolithic
    form and rank 0 holds the line; here rank 1 of a two-rank run through the production branch (test double of librccl) never enters the
    probe (TPG_BENCH_TEST_STALL_PIPELINED): the soft watchdog must print ONE diagnostic per rank on stderr, rank 0 must still print the
    contract line -- the monolithic form's, `pipelined_probe.status == "stalled"`, no pipelined figures -- and the job must leave with
    status 9 (a hang inside a product entry point is not a successful run; the line is out, the status says so)."""
    env = dict(os.environ, TPG_BENCH_REHEARSE="shim", MASTER_ADDR="127.0.0.1", TPG_BENCH_TEST_STALL_PIPELINED="1", TPG_SHIM_DEADLINE_S="120")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TPG_RCCL_LIBRARY"):
        env.pop(k, None)
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--preroll", "8", "--deadline", "10"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 9 and time.time() - t0 < 200, (p.returncode, p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["pipelined_probe"]["status"] == "stalled" and "pipelined probe (pipelined_1)" in d["pipelined_probe"]["phase"]
    assert d["pipelined_probe"]["exit_status"] == 9
    assert d["exchange_form"] == "monolithic" and d["exchange_ms_monolithic"] > 0 and d["exchange_ms_pipelined_1"] is None
    assert d["ms_per_step_by_form"] == {"monolithic": d["ms_per_step"]} and all(r["seams_bit_exact"] for r in d["per_rank"])
    diag = [json.loads(l[l.index("{"):]) for l in p.stderr.splitlines() if "pipelined_probe_stalled" in l]
    assert {x["rank"] for x in diag} == {0, 1}


def test_bench_wrong_seams_from_a_pipelined_form_fail_the_job_after_the_line(gpu):
    """a pipelined form that delivers halos which are not bit-exact (here: one received cell altered on rank 0 right
    before the probe's seam verification, TPG_BENCH_TEST_CORRUPT_PIPELINED_SEAM) must not be recorded as a successful run.  The monolithic
    line is still printed -- with `pipelined_probe.status == "seam_mismatch"` and no figures for the failed form --, a `seam_mismatch`
    diagnostic names side and field on stderr, and EVERY rank leaves with status 9."""
    env = dict(os.environ, TPG_BENCH_REHEARSE="shim", MASTER_ADDR="127.0.0.1", TPG_BENCH_TEST_CORRUPT_PIPELINED_SEAM="0", TPG_SHIM_DEADLINE_S="60")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TPG_RCCL_LIBRARY"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--preroll", "8"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 9, (p.returncode, p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), p.stdout[-2000:]
    d = json.loads(lines[0])
    pp = d["pipelined_probe"]
    assert pp["status"] == "seam_mismatch" and pp["exit_status"] == 9 and set(pp["forms"].values()) == {"seam_mismatch"}
    assert d["exchange_form"] == "monolithic" and d["exchange_ms_pipelined_1"] is None and d["exchange_ms_pipelined_2"] is None
    assert all(r["seams_bit_exact"] for r in d["per_rank"])                     # the monolithic run itself was verified and stands
    diag = [json.loads(l[l.index("{"):]) for l in p.stderr.splitlines() if '"seam_mismatch"' in l and l.lstrip().startswith("{")]
    assert diag and all(x["rank"] == 0 and x["bit_exact"] is False and x["exit_status"] == 9 for x in diag)
    assert {x["form"] for x in diag} == {"pipelined_1", "pipelined_2"}


def test_bench_stalled_teardown_is_reported(gpu):
    """A communicator / process-group shutdown that never returns (TPG_BENCH_TEST_STALL_TEARDOWN on rank 1 of a two-rank rehearsal, 3 s
    limit): the contract line is already out, the job still exits 0 -- and rank 1 says on stderr which call it was stuck in."""
    env = dict(os.environ, TPG_BENCH_REHEARSE="1", MASTER_ADDR="127.0.0.1", TPG_BENCH_TEST_STALL_TEARDOWN="1", TPG_BENCH_TEARDOWN_S="3")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len([l for l in p.stdout.splitlines() if l.startswith('{"metric"')]) == 1
    diag = [json.loads(l) for l in p.stderr.splitlines() if l.startswith("{") and "teardown_stalled" in l]
    d1 = [x for x in diag if x["rank"] == 1]
    assert len(d1) == 1 and d1[0]["phase"] == "teardown" and "destroy" in d1[0]["pending_call"] and d1[0]["exit_status"] == 0


@pytest.mark.parametrize("band", [3, 7])
def test_bench_loopback_runs_the_rccl_branch(gpu, band):
    """`bench.py --loopback`: the `comm is not None` branch of bench.py on a one-GPU box -- RcclComm bring-up under the watchdog,
    seam buffers, tpg_fill_halo_regions_distributed_peers AND its pipelined form (first contact, pre-pass, timed steps on the side
    stream beside the build, instrumented passes), for band 3 of 8 (interior: two seams) and band 7 of 8 (zipper + south seam) of
    BASELINE config 4.  Both peers are the rank itself: no link, no scaling claim -- the line must say so."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TPG_BENCH_REHEARSE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--loopback", "--loopback-band", str(band), "--steps", "6", "--warmup", "2"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["config"]["rows_per_rank"] == 225 and "LOOP-BACK" in d["config"]["workload"]
    assert d["loopback"] == {"bands": 8, "band": band, "south_peer": 0, "north_peer": 0 if band < 7 else -1, "zipper": band == 7}
    assert "librccl" in d["exchange_transport"] and "loop-back" in d["exchange_transport"] and "rehearsal" in d["note"]
    forms = {"monolithic", "pipelined_1", "pipelined_2"}
    assert d["exchange_ms_monolithic"] > 0 and d["exchange_ms_pipelined_1"] > 0 and d["exchange_ms_pipelined_2"] > 0 and d["exchange_form"] in forms
    assert d["exchange_ms"] == d["exchange_ms_" + d["exchange_form"]]
    assert d["exchange_ms_pipelined"] == min(d["exchange_ms_pipelined_1"], d["exchange_ms_pipelined_2"])
    assert set(d["exchange_prepass_fill_ms"]) == forms
    assert abs(d["value"] - 3600 * 225 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]                # this band's cells only
    pr = d["per_rank"]
    assert len(pr) == 1 and pr[0]["band"] == band and pr[0]["seams"] == (2 if band < 7 else 1) and pr[0]["zipper"] == (band == 7)
    assert pr[0]["rows"] == [225 * band + 1, 225 * band + 225] and set(pr[0]["exchange_ms_by_form"]) == forms
    assert (d["roofline"]["launch_ms"] > 0) == (band == 7)                                               # only the zipper band launches the merged fold
    assert d["roofline_precompute"]["evaluated_cells"] == 3600 * (233 if band < 7 else 229)
    assert "cpu_baseline" not in d and "fill_step" not in d
    # the seams were verified bit for bit against the neighbour's rebuilt field (here: this band's own) before anything was timed
    assert pr[0]["seams_bit_exact"] is True and "bit for bit" in d["seam_check"]


def test_bench_seam_check_has_teeth(gpu):
    """One received halo cell altered after the first exchanges (TPG_BENCH_TEST_CORRUPT_SEAM): the seam verification must end the run
    with exit status 6, a `seam_mismatch` diagnostic naming side and field on stderr, and no contract line."""
    env = dict(os.environ, TPG_BENCH_TEST_CORRUPT_SEAM="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TPG_BENCH_REHEARSE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--loopback", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 6 and not p.stdout.strip(), (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    diag = [json.loads(l) for l in p.stderr.splitlines() if l.startswith("{") and "seam_mismatch" in l]
    assert len(diag) == 1 and diag[0]["bit_exact"] is False and len(diag[0]["bad"]) == 1
    bad = diag[0]["bad"][0]
    assert (bad["side"], bad["field"], bad["cells"]) == ("south", "u", 1) and bad["first_level_row_col"] == [37, 3, 1800]


def test_bench_deadline_fires_with_a_diagnostic(gpu):
    """A stalled first exchange must end the job loudly: rank 1 of a two-rank rehearsal is told (TPG_BENCH_TEST_STALL_RANK) to sleep
    instead of entering its first fill, so rank 0 blocks in the gloo exchange; with a 10 s deadline rank 0 prints the one-line JSON
    diagnostic (rank, peers, phase) on stderr and the job exits non-zero -- no JSON line on stdout.  Launched WITHOUT a launcher:
    bench.py's own parent must pass the failure on (non-zero exit) and stop the sleeping worker."""
    env = dict(os.environ, TPG_BENCH_REHEARSE="1", MASTER_ADDR="127.0.0.1", TPG_BENCH_TEST_STALL_RANK="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--deadline", "10"]
    t0 = time.time()
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode != 0 and time.time() - t0 < 200
    assert not [l for l in p.stdout.splitlines() if l.strip().startswith('{"metric"')]
    diag = [json.loads(l[l.index("{"):]) for l in p.stderr.splitlines() if "bench_deadline_expired" in l]
    assert diag, p.stderr[-3000:]
    d0 = [d for d in diag if d["rank"] == 0][0]
    assert d0["world"] == 2 and d0["peers"] == {"south": None, "north": 1} and "first seam exchange" in d0["phase"] and d0["deadline_s"] == 10
