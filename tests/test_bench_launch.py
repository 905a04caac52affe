"""bench.py's launch paths on the CPU: `python bench.py --gpus N` must start N fresh ranks by itself (the driver's
scaling run may call it without torch.distributed.run), the torchrun form must keep working, and a launch that cannot
work must fail fast with a message instead of producing nothing.  --rendezvous-only forms the process group (gloo) and
reports what it saw; no GPU work."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                             "EVDR_BENCH_LAUNCHER")}
    return env


def _last_json(out: str):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out                      # exactly ONE line, from rank 0
    return json.loads(lines[0])


def test_self_launch_forms_world_of_n():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--rendezvous-only"], capture_output=True, text=True, timeout=300,
                       env=_clean_env())
    assert r.returncode == 0, r.stderr
    rec = _last_json(r.stdout)
    assert rec == {"rendezvous": "ok", "world_size": 3, "ranks_seen": 3, "launcher": "self"}
    assert r.stdout.strip().count("\n") == 0 and r.stdout.strip().startswith("{")      # stdout carries the JSON line and nothing else (Gloo's own chatter goes to stderr)


def test_torchrun_form_still_works():
    port = 29900 + os.getpid() % 90
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--rendezvous-only"],
                       capture_output=True, text=True, timeout=300, env=_clean_env())
    assert r.returncode == 0, r.stderr
    rec = _last_json(r.stdout)
    assert rec["world_size"] == 2 and rec["ranks_seen"] == 2 and rec["launcher"] == "torchrun"


def test_single_rank_needs_no_launcher():
    r = subprocess.run([sys.executable, BENCH, "--rendezvous-only"], capture_output=True, text=True, timeout=300, env=_clean_env())
    assert r.returncode == 0 and _last_json(r.stdout)["world_size"] == 1


def test_world_size_mismatch_and_missing_gpus_fail_loudly():
    env = dict(_clean_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--rendezvous-only"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300, env=_clean_env())
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and r.stdout.strip() == ""
    import torch
    if torch.cuda.device_count() < 8:
        r = subprocess.run([sys.executable, BENCH, "--gpus", "8"], capture_output=True, text=True, timeout=300, env=_clean_env())
        assert r.returncode == 2 and "visible GPUs" in r.stderr and r.stdout.strip() == ""


def test_committed_bench_line_follows_the_contract():
    """The last committed bench line (profiles/r06_bench_n1.json, written by `python bench.py` on an MI355X) carries every field
    the driver's contract names, the roofline object of the dominant kernel, the CPU baseline, the training-step, evaluation and
    phase records (round 3), since round 4 kernel times taken inside the timed steps and inside the training step, since
    round 5 the counter traffic of the three training kernels and the configs[4] step parity at N = 500 in the training record, and
    since round 6 the basis of every roofline figure (means, the minimum only beside them), the configs[2] record in both dtypes and
    the unmodified call pattern with the frozen-teacher score cache on."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_n1.json")))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in rec, key
    assert rec["n_gpus"] == 1 and rec["higher_is_better"] is True and rec["vs_baseline"] is None and rec["data"] == "synthetic"
    assert "workload" in rec["config"] and "model" not in rec["config"]
    assert abs(rec["value"] - rec["config"]["pages"] * rec["config"]["queries_per_step"] / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    r = rec["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert abs(r["achieved"] - r["algorithmic_flop_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e12) < 1e-6 * r["achieved"]
    assert r["kernel"].startswith("maxsim_fwd16s_kernel<") and r["kernel_ms"] <= rec["ms_per_step"]
    assert r["traffic"] is None or r["traffic_source"]["file"] == "profiles/hbm_traffic.json"
    if r["traffic"] is not None:
        # the replayed counter figure is the committed file's (hash recorded in the line), taken for THIS kernel symbol and
        # launch shape, and agrees with the rocprofv3 summary it was derived from
        import hashlib
        raw = open(os.path.join(ROOT, "profiles", "hbm_traffic.json"), "rb").read()
        assert hashlib.sha256(raw).hexdigest().startswith(r["traffic_source"]["sha256"])
        t = json.loads(raw)
        assert t["kernel"] == r["kernel"] and t["queries"] == rec["config"]["queries_per_step"] and t["pages_per_gpu"] == rec["config"]["pages"]
        assert r["traffic"] == t["hbm_bytes_per_launch"] >= r["algorithmic_bytes_per_launch"]
        pmc = json.load(open(os.path.join(ROOT, "profiles", "r06_pmc_summary.json")))
        assert pmc["hbm_bytes_per_launch"] == t["hbm_bytes_per_launch"]
    assert "INSIDE the timed region" in r["kernel_ms_basis"] or "inside the timed region" in r["kernel_ms_basis"]
    stats = open(os.path.join(ROOT, "profiles", "r06_bench_kernel_stats.csv")).read().splitlines()
    top = next(ln for ln in stats[1:] if "maxsim_fwd16s_kernel<4, 1, false, 8" in ln)
    avg_ms = float(top.split('",')[1].split(",")[2]) / 1e6
    assert abs(avg_ms - r["kernel_ms"]) < 0.01 * r["kernel_ms"]           # rocprofv3's average agrees with the HIP-event time of the line
    for o in r["other_regimes"]:
        assert o["bound"] == "hbm" and o["peak"] == 8000.0 and 0.3 < o["frac"] < 1.0
        # round 6: the figure is the MEAN of the launches (what rocprofv3's average reports), the minimum rides beside it
        assert "mean of" in o["kernel_ms_basis"] and o["kernel_ms_min"] <= o["kernel_ms"]
        assert abs(o["frac"] - o["algorithmic_bytes_per_launch"] / (o["kernel_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
        sym = o["kernel"].rstrip(">").replace(",", ", ")                  # (the listing carries one more, defaulted, template argument)
        row = next(ln for ln in stats[1:] if sym in ln)
        avg = float(row.split('",')[1].split(",")[2]) / 1e6
        assert abs(avg - o["kernel_ms"]) < 0.08 * o["kernel_ms"], (o["kernel"], avg, o["kernel_ms"])   # rocprofv3's average of the same command
    # round 6: BASELINE.json configs[2] through the drop-in API, bf16 and the reference's own dtype
    c2 = rec["configs2"]
    assert c2["config"]["queries"] == 500 and c2["config"]["pages"] == 6847
    for name, products in (("bf16", 1), ("fp32", 3)):
        e_ = c2[name]
        rr = e_["roofline"]
        assert e_["planted_top1"] == 1.0 and abs(e_["pairs_per_s"] - 500 * 6847 / (e_["call_ms"] * 1e-3)) < 1e-6 * e_["pairs_per_s"]
        assert rr["executed_flop_per_launch"] == products * rr["algorithmic_flop_per_launch"] == products * 500 * 6847 * 2 * 32 * 1030 * 128
        assert abs(rr["frac"] - rr["executed_flop_per_launch"] / (rr["kernel_ms"] * 1e-3) / 1e12 / 2500.0) < 1e-9
        assert abs(rr["frac_algorithmic"] * products - rr["frac"]) < 1e-9 and rr["kernel_ms_min"] <= rr["kernel_ms"] <= e_["call_ms"] * 1.02
        assert rr["kernel"].startswith("maxsim_fwd16s_kernel<4,1,false,8" if name == "bf16" else "maxsim_fwd16s_kernel<2,2,false,4") and "mean of" in rr["kernel_ms_basis"]
    assert c2["fp32"]["pairs_per_s"] < c2["bf16"]["pairs_per_s"] < 1.1 * rec["value"]
    c = rec["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "pairs/s" and c["cores"] >= 1 and c["max_abs_diff_vs_gpu"] < 1e-4
    assert "median of 3" in c["sample"] and "2048 pages" in c["sample"]
    # round 3: the training half (configs[4]), the evaluation (configs[1]) and the phase split ride in the same line
    t = rec["train_step"]
    assert set(t["results"]) == {"call_pattern", "call_pattern_cached", "fused", "fused_cached"} and t["config"]["pages"] == 500
    # round 6: the reference's unmodified step with evaluator.retrieval.enable_score_cache() -- the frozen teacher's
    # forward (0.265 ms of the step) is gone after the first epoch; what is left is host-bound on slow boxes
    cpc = t["results"]["call_pattern_cached"]
    assert cpc["ms_per_step"] < t["results"]["call_pattern"]["ms_per_step"] - 0.12 and cpc["score_cache"]["entries"] == 64 * 32
    for r_ in t["roofline"][:2]:
        assert r_["executed_flop_per_launch"] == 3 * r_["algorithmic_flop_per_launch"] and "EXECUTED" in r_["frac_basis"]
        assert abs(r_["frac"] - r_["executed_flop_per_launch"] / (r_["kernel_ms"] * 1e-3) / 1e12 / 2500.0) < 1e-9
        assert abs(r_["algorithmic_tflops"] - r_["algorithmic_flop_per_launch"] / (r_["kernel_ms"] * 1e-3) / 1e12) < 1e-6
    assert t["roofline"][2]["bound"] == "hbm" and t["cpu_baseline"]["kind"] == "port" and t["cpu_baseline"]["sample_pages"] <= 500
    # round 5: the timed step is the production path; every training kernel's roofline carries the replayed counter traffic (close to
    # its algorithmic bytes: nothing is re-read); the oracle step at the bench's own N = 500 is compared with the fused GPU step
    assert "PageCorpus.topk" in rec["timed_path"]
    for e_ in t["roofline"]:
        assert e_["traffic_source"]["file"] == "profiles/train_traffic.json" and 1.0 <= e_["traffic_over_algorithmic"] < 1.15, e_["role"]
    import hashlib
    raw_t = open(os.path.join(ROOT, "profiles", "train_traffic.json"), "rb").read()
    assert hashlib.sha256(raw_t).hexdigest().startswith(t["roofline"][0]["traffic_source"]["sha256"])
    cb = t["cpu_baseline"]
    assert cb["sample_pages"] == 500 and cb["loss_rel_diff_vs_gpu"] <= 1e-5 and cb["grad_max_abs_diff_vs_gpu"] <= 1e-6
    assert cb["param_max_abs_diff_vs_gpu"] <= 1e-6 and cb["param_max_abs_diff_vs_adamw_of_gpu_gradient_all_entries"] <= 1e-6
    assert cb["argmax_mismatches"] == 0 and cb["teacher_target_mismatches"] == 0
    # round 4: every training kernel is stated alone AND inside the step; the in-step figures add up to less than the step, and each
    # agrees within 3 % ... 8 % box noise with the rocprofv3 trace of the timed steps of the same call
    trace = json.load(open(os.path.join(ROOT, "profiles", "r06_train_fused_trace_exclusive.json")))
    assert trace["last_calls_per_kernel"] == 30
    assert sum(v["overlap_with_predecessor_avg_us"] for v in trace["kernels"].values()) < 1.0      # intervals of one queue do not overlap
    keys = ("maxsim_fwd16s_kernel<2, 2, false", "maxsim_fwd16s_kernel<2, 2, true", "maxsim_bwd_kernel")
    in_step = [r_["kernel_ms_in_step"] for r_ in t["roofline"]]
    # the brackets (HIP events around each launch, the launch gap in front of it included) add up to less than the step they were taken in;
    # that instrumented step is within 10 % of the plain one (since round 4's second session the step launches little else: the three
    # kernels and the 7-us loss)
    import re
    with_events = float(re.search(r"step with the events ([0-9.]+) ms", t["roofline"][0]["kernel_ms_in_step_basis"]).group(1))
    assert sum(in_step) < with_events < 1.10 * t["results"]["fused"]["ms_per_step"]
    prof_step = json.load(open(os.path.join(ROOT, "profiles", "r06_prof_train_line.json")))["results"]["fused"]["ms_per_step"]
    # per step: the step's own kernels (30 calls each in the 30 timed steps) plus the once-per-epoch preparation (driver.EpochBatches:
    # two gathers and one split launch per epoch, a few calls in the whole trace) spread over the steps
    per_step_us = sum(v["plain_avg_us"] * min(v["calls"], 30) / 30.0 for v in trace["kernels"].values())
    assert per_step_us * 1e-3 < prof_step + 0.005
    assert trace["kernels"]["split_segments_kernel"]["calls"] <= 3 and "split_small_kernel" not in trace["kernels"]   # no per-step split / gather
    for k_, ms_, r_ in zip(keys, in_step, t["roofline"]):
        us = trace["kernels"][k_]["plain_avg_us"]
        assert abs(us * 1e-3 - ms_) < 0.08 * ms_, (k_, us, ms_)
        assert "alone" in r_["kernel_ms_basis"] and "inside the fused step" in r_["kernel_ms_in_step_basis"]
        assert abs(r_["frac_in_step"] * r_["kernel_ms_in_step"] - r_["frac"] * r_["kernel_ms"]) < 1e-9
    e = rec["eval"]
    for name in ("bf16", "fp32"):
        assert e[name]["ndcg_at_5"] == 1.0 and e[name]["device_ms"] + e[name]["d2h_ms"] + e[name]["host_ms"] <= e[name]["total_ms"]
    assert e["bf16"]["total_ms"] <= 5.0                                   # configs[1] end to end
    ph = rec["phases"]
    assert set(ph["rank0"]) == {"score_ms", "topk_ms"} and abs(ph["rank0"]["score_ms"] - r["kernel_ms"]) < 0.02 * r["kernel_ms"]
    assert rec["dist"]["ranks_seen"] == 1 and rec["dist"]["pages_per_rank"] == rec["config"]["pages"]
    # and the standalone training bench of the same call agrees with the line's record within box noise
    bt = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_train.json")))
    for mode in ("call_pattern", "call_pattern_cached", "fused", "fused_cached"):
        assert abs(bt["results"][mode]["ms_per_step"] - t["results"][mode]["ms_per_step"]) < 0.08 * bt["results"][mode]["ms_per_step"]
