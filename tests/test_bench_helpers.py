"""CPU tests of bench.py's host logic: the live-traffic probe (rocprofv3 --pmc child runs) against a stand-in profiler, and the
stage model / byte formulas the roofline block is computed from."""
import importlib.util
import os
import stat
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FAKE = textwrap.dedent('''\
    #!%s
    # stand-in for rocprofv3: writes a counter_collection.csv like the real tool (one row per counter, dispatch and XCD instance)
    import os, sys
    a = sys.argv[1:]
    cut = a.index("--")
    opts = a[:cut]
    counters = []
    i = opts.index("--pmc") + 1
    while i < len(opts) and not opts[i].startswith("-"):
        counters.append(opts[i]); i += 1
    d = opts[opts.index("-d") + 1]
    if os.environ.get("FAKE_ROCPROF_FAIL"):
        sys.stderr.write("boom\\n"); sys.exit(3)
    assert os.environ.get("GACQ_BENCH_PMC_CHILD") == "1" and "RANK" not in os.environ
    os.makedirs(os.path.join(d, "host"), exist_ok=True)
    with open(os.path.join(d, "host", "p_counter_collection.csv"), "w") as f:
        f.write("Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value\\n")
        for disp in (1, 2, 3):
            for c in counters:
                for xcd in range(8):                      # per-XCD instances of one dispatch are summed
                    f.write('%%d,"void (anonymous namespace)::lds_fused4k_kernel<4, true>(float2 const*)",%%s,%%d\\n' %% (disp, c, 100 * disp))
                f.write('%%d,"(anonymous namespace)::best_doppler_kernel(RowRec const*)",%%s,7\\n' %% (disp, c))
    ''') % sys.executable


def test_pmc_passes_reads_one_counter_group_per_child_run(bench, tmp_path, monkeypatch):
    exe = tmp_path / "rocprofv3"
    exe.write_text(FAKE)
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr("shutil.which", lambda name: str(exe) if name == "rocprofv3" else None)
    monkeypatch.setenv("RANK", "0")                       # a torchrun parent's rendezvous variables must not reach the child
    got = bench.pmc_passes(["--steps", "3"], "lds_fused4k_kernel", [["FETCH_SIZE"], ["WRITE_SIZE"], ["GRBM_GUI_ACTIVE", "SQ_ACTIVE_INST_VALU"]])
    # dispatches 1, 2, 3 -> 8 instances x 100 x id each; the average per launch is 8 * 100 * 2
    assert got["FETCH_SIZE"] == 1600.0 and got["WRITE_SIZE"] == 1600.0 and got["SQ_ACTIVE_INST_VALU"] == 1600.0
    assert got["launches"] == 3
    with pytest.raises(RuntimeError, match="no FETCH_SIZE rows"):
        bench.pmc_passes([], "some_other_kernel", [["FETCH_SIZE"]])


def test_pmc_passes_reports_a_failing_profiler(bench, tmp_path, monkeypatch):
    exe = tmp_path / "rocprofv3"
    exe.write_text(FAKE)
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr("shutil.which", lambda name: str(exe) if name == "rocprofv3" else None)
    monkeypatch.setenv("FAKE_ROCPROF_FAIL", "1")
    with pytest.raises(RuntimeError, match="rc 3"):
        bench.pmc_passes([], "lds_fused4k_kernel", [["FETCH_SIZE"]])


def test_stage_boundary_byte_model_matches_survey_8d(bench):
    # config 2 of SURVEY.md 8d: P = 32, D = 40, B = 1, N = 4096 -> A_pipe = 216.0 MB; config 1: 5.9 MB
    assert bench.a_pipe_bytes(4096, 32, 40, 1) == 8 * 4096 * (4 * 40 + 32 + 5 * 32 * 40)
    assert round(bench.a_pipe_bytes(4096, 32, 40, 1) / 1e6, 1) == 216.0
    assert round(bench.a_pipe_bytes(4096, 1, 20, 1) / 1e6, 1) == 5.9
    # B > 1 adds the fp32 q read + write per extra block; GLONASS has one forward set per channel
    assert bench.a_pipe_bytes(16384, 15, 200, 10, F=15) - bench.a_pipe_bytes(16384, 15, 200, 10, F=1) == 8 * 16384 * 4 * 200 * 10 * 14
    assert bench.engine_kind(4096) == "lds" and bench.engine_kind(61380) == "split31" and bench.engine_kind(65536) == "split_lds"


def _records(bench, E, P, seed):
    import numpy as np
    from gnss_dsp_tools_amd import acquire
    rng = np.random.default_rng(seed)
    r = np.zeros((E, P), dtype=acquire.PEAK_DTYPE)
    r["metric"] = rng.random((E, P)) * 10.0
    r["idx"] = rng.integers(0, 4096, (E, P))
    r["d_index"] = rng.integers(-1, 40, (E, P))
    return r


def test_dump_outputs_writes_every_record_field_as_float64(bench, tmp_path):
    import numpy as np
    jobs = [{"label": "gps-l1"}, {"label": "galileo-e1b+galileo-e1c"}]
    recs = [_records(bench, 4, 32, 1), _records(bench, 4, 72, 2)]
    bench.dump_outputs(str(tmp_path), jobs, recs)
    assert sorted(os.listdir(tmp_path)) == sorted("%s_%s.npy" % (j["label"], f) for j in jobs for f in ("metric", "code_index", "doppler_index"))
    for j, r in zip(jobs, recs):
        for field, name in (("metric", "metric"), ("idx", "code_index"), ("d_index", "doppler_index")):
            a = np.load(tmp_path / ("%s_%s.npy" % (j["label"], name)))
            assert a.dtype == np.float64 and a.shape == r.shape and np.array_equal(a, r[field])


def test_dump_outputs_above_the_cap_keeps_the_same_seeded_sample_of_epochs(bench, tmp_path, monkeypatch):
    import numpy as np
    jobs = [{"label": "a"}, {"label": "b"}]
    recs = [_records(bench, 200, 32, 3), _records(bench, 100, 16, 4)]
    total = sum(r.size * 3 * 8 for r in recs)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", total // 4)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), jobs, recs)
    written = sum(os.path.getsize(tmp_path / "x" / f) - 128 for f in os.listdir(tmp_path / "x") if not f.endswith("_epoch.npy"))
    assert 0 < written <= total // 4
    for j, r in zip(jobs, recs):
        ep = np.load(tmp_path / "x" / ("%s_epoch.npy" % j["label"]))
        assert np.array_equal(ep, np.load(tmp_path / "y" / ("%s_epoch.npy" % j["label"])))          # fixed sample
        assert len(ep) >= 1 and np.all(np.diff(ep) > 0) and ep[-1] < r.shape[0]
        m = np.load(tmp_path / "x" / ("%s_metric.npy" % j["label"]))
        assert np.array_equal(m, r["metric"][ep.astype(int)])


def test_dump_outputs_of_the_launch_path_one_rank_equals_two_ranks(tmp_path):
    """bench.py --dump-outputs through the --dry-run-cpu launch path (the per-rank compute stood in by the oracle): the same arguments
    give the same files; two ranks over gloo (Doppler slices, exchange, merge) dump what one rank computes over the whole grid."""
    import json
    import socket
    import subprocess
    import numpy as np
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    common = [os.path.join(ROOT, "bench.py"), "--config", "2", "--steps", "3", "--warmup", "1", "--scaling", "strong", "--epochs", "2",
              "--dry-run-cpu", os.path.join(ROOT, "tests", "_gloo_worker.py") + ":oracle_local"]
    runs = {"one": [sys.executable] + common, "again": [sys.executable] + common,
            "two": [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(port)] + common + ["--gpus", "2"]}
    for name, cmd in runs.items():
        details = tmp_path / ("%s.json" % name)
        out = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / name), "--details-json", str(details)], capture_output=True, text=True,
                             timeout=600, cwd=ROOT)
        assert out.returncode == 0, (name, out.stderr[-3000:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == 3, lines
        assert json.load(open(details)) == json.loads(lines[0])              # no side runs here: the record is the line
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == ["gps-l1_code_index.npy", "gps-l1_doppler_index.npy", "gps-l1_metric.npy"]
    for name in ("again", "two"):
        assert sorted(os.listdir(tmp_path / name)) == files
        for f in files:
            a, b = np.load(tmp_path / "one" / f), np.load(tmp_path / name / f)
            assert a.dtype == np.float64 and a.shape == (2, 3) and np.array_equal(a, b), (name, f, a, b)
    assert (np.load(tmp_path / "one" / "gps-l1_metric.npy") > 0).all()


def test_result_line_cuts_the_side_runs_to_their_headline_numbers_and_keeps_the_rest(bench):
    import json
    prose = "x" * 400
    out = {"metric": "m", "value": 1.5e12, "ms_per_step": 5.2, "steps": 20, "roofline": {"model": prose, "frac": 0.5}, "bench_wall_s": 80.0,
           "other_configs": [{"baseline_config": k, "workload": prose, "value": 1e11 * k, "ms_per_step": float(k), "bound": "hbm", "frac": 0.5,
                              "stream_ceiling": {"all": [prose]}} for k in (3, 4, 5)] + [{"baseline_config": 6, "error": "boom"}],
           "reference_precision": {"engine": prose, "dtype": "f64", "value": 4e11, "ms_per_step": 13.0, "f32_over_f64": 2.4, "roofline": {"note": prose},
                                   "other_configs": [{"baseline_config": 3, "value": 1e11, "ms_per_step": 4.6, "f32_over_f64": 2.4, "roofline": {"model": prose}}]},
           "next_rows": {"frontend": {"what": prose, "ms": 0.1, "calls_timed": 5000}, "longcode_l2cl": {"ms": 0.08, "k_found": 37, "k_injected": 37},
                         "tracking_epl": {"what": prose, "us_resident_block": 16.0}}}
    line = bench.result_line(out)
    assert set(line) == set(out) and "other_configs" in out and len(out["other_configs"]) == 4          # the record itself is untouched
    for k in ("metric", "value", "ms_per_step", "steps", "roofline", "bench_wall_s"):
        assert line[k] == out[k]
    assert line["other_configs"] == [{"baseline_config": k, "value": 1e11 * k, "ms_per_step": float(k), "bound": "hbm", "frac": 0.5} for k in (3, 4, 5)] + \
        [{"baseline_config": 6, "error": "boom"}]
    assert line["reference_precision"] == {"dtype": "f64", "value": 4e11, "ms_per_step": 13.0, "f32_over_f64": 2.4,
                                           "other_configs": [{"baseline_config": 3, "value": 1e11, "ms_per_step": 4.6, "f32_over_f64": 2.4}]}
    assert line["next_rows"] == {"frontend": {"ms": 0.1}, "longcode_l2cl": {"ms": 0.08, "k_found": 37, "k_injected": 37}, "tracking_epl": {"us_resident_block": 16.0}}
    assert bench.result_line({"next_rows": {"error": "e"}, "reference_precision": {"error": "f"}}) == {"next_rows": {"error": "e"}, "reference_precision": {"error": "f"}}
    assert len(json.dumps(line)) < len(json.dumps(out)) - 10 * len(prose)          # 11 prose strings of the side runs dropped, 1 (roofline) kept
    plain = {"metric": "m", "value": 1.0, "config": {"workload": prose}}
    assert bench.result_line(plain) == plain                                                            # no side runs: the line is the record
