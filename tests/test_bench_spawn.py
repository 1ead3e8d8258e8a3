"""`python bench.py --gpus N` as typed: the parent starts its own ranks (no launcher).  On the CPU the same spawner and
rank program run through tests/bench_dry.py (gloo, tests/dry_device.py in place of the GPU); on a GPU box `--gpus 1` goes
through the real path.  bench.py itself has no dry switch."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRY = os.path.join("tests", "bench_dry.py")


def _run(args, timeout=900, script="bench.py"):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    return p


def _line(p):
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0])


def test_two_ranks_started_by_the_bench_itself_dry():
    d = _line(_run(["--gpus", "2", "--reads", "3000", "--steps", "3", "--warmup", "1", "--full"], script=DRY))
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and len(d["config"]["devices"]) == 2
    assert d["dry_run"] is True and d["value"] is None            # a dry run never carries a rate
    assert d["scaling"] == "weak" and d["gather"]["tuple_bytes"] == 5
    assert d["gather"]["ms_per_step_without_gather"] is not None


def test_config4_fixed_total_sharded_dry():
    # 10 001 reads over 2 ranks in steps of 2 000: shards of 5 000 / 5 001 reads -> 3 steps each, the last ones short
    d = _line(_run(["--gpus", "2", "--config", "4", "--total-reads", "10001", "--reads", "2000", "--warmup", "1"], script=DRY))
    assert d["scaling"] == "strong" and d["steps"] == 3 and d["n_gpus"] == 2
    assert "10001" in d["config"]["workload"]
    assert 0.3 < d["config"]["decombined_fraction"] < 0.5


def test_eight_ranks_config4_uneven_total_dry():
    # BASELINE config 4's world size: 16 001 reads over 8 ranks in steps of 2 000 -> shards of 2 000 and (one) 2 001 reads:
    # one rank needs a second step for its last read, the other seven run an empty trailing step; every rank's message is
    # checked against its count on rank 0 (TupleGather.check), the line names the world and every rank's own step time
    d = _line(_run(["--gpus", "8", "--config", "4", "--total-reads", "16001", "--reads", "2000", "--warmup", "1", "--full"], script=DRY))
    assert d["scaling"] == "strong" and d["steps"] == 2 and d["n_gpus"] == 8 and d["world_size"] == 8
    assert len(d["per_rank_ms_per_step"]) == 8 and len(d["config"]["devices"]) == 8
    assert d["gather"]["tuple_bytes"] == 5 and d["gather"]["exposed_ms_per_step"] is not None
    assert 0.3 < d["config"]["decombined_fraction"] < 0.5


def test_a_plain_run_leaves_the_extra_loops_to_full_dry():
    # without --full the line carries the headline only: no gather A/B loop, no CPU baseline (the keys are there, null)
    d = _line(_run(["--gpus", "2", "--reads", "3000", "--steps", "4", "--warmup", "1"], script=DRY))
    assert d["full"] is False and d["steps"] == 4 and d["cpu_baseline"] is None and d["ms_per_step_steady"] is None
    assert d["gather"]["ms_per_step_without_gather"] is None and d["gather"]["exposed_ms_per_step"] is None


def _load_dump(d):
    import numpy as np
    out = {}
    for name in sorted(os.listdir(d)):
        assert name.endswith(".npy"), name
        out[name[:-4]] = np.load(os.path.join(d, name))
    return out


@pytest.mark.parametrize("config,chains", [(2, 1), (3, 2)])
def test_dump_outputs_dry(tmp_path, config, chains):
    """--dump-outputs on the dry rank program: the last step's records (all 3 000 reads: below the sample size) and counters of
    every chain, float32 / float64, the same in a second run with the same arguments."""
    import numpy as np
    from decombinator_amd import _native as nat
    dumps = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        line = _line(_run(["--gpus", "1", "--config", str(config), "--reads", "3000", "--steps", "3", "--warmup", "1",
                           "--dump-outputs", str(d)], script=DRY))
        assert sorted(line["dumped_outputs"]) == sorted(x[:-4] for x in os.listdir(d))
        dumps.append(_load_dump(d))
    a, b = dumps
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert np.array_equal(a["sample_index"], np.arange(3000))
    tags = [""] if chains == 1 else [f"chain{c}_" for c in range(chains)]
    for c, tag in enumerate(tags):
        cnt = a["counters" + (f"_chain{c}" if chains > 1 else "")]
        assert cnt[nat.COUNTER_NAMES.index("read_count")] == 3000
        status = a[f"records_{tag}status"]
        assert set(a) >= {f"records_{tag}{f}" for f in nat.RECORD_DTYPE.names}
        assert cnt[nat.COUNTER_NAMES.index("vj_count")] == (status == 0).sum() > 500


def test_dump_outputs_samples_a_large_step(tmp_path):
    """A step of more reads than the sample holds: the same sorted sample of indices in every run, the records at those
    indices field by field, at most 64 MB in all — for one chain and for two."""
    import numpy as np
    import bench
    from decombinator_amd import _native as nat
    n = 3_000_000
    rng = np.random.default_rng(5)
    rec = np.zeros(n, dtype=nat.RECORD_DTYPE)
    for f in nat.RECORD_DTYPE.names:
        rec[f] = rng.integers(0, 255 if rec[f].dtype == np.uint8 else 65535, n)
    cnt = np.arange(nat.N_COUNTERS, dtype=np.uint64) * 1000
    for chains in (1, 2):
        got = []
        for k in range(2):
            d = str(tmp_path / f"c{chains}_{k}")
            names = bench.dump_outputs(d, [(rec, cnt)] * chains)
            got.append(_load_dump(d))
            assert sorted(names) == sorted(got[-1])
        a, b = got
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert sum(os.path.getsize(os.path.join(tmp_path / f"c{chains}_0", x)) for x in os.listdir(tmp_path / f"c{chains}_0")) <= 64 << 20
        idx = a["sample_index"]
        assert idx.dtype == np.float64 and len(idx) == bench.DUMP_SAMPLE_READS // chains
        assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
        tag = "" if chains == 1 else "chain1_"
        for f in nat.RECORD_DTYPE.names:
            assert a[f"records_{tag}{f}"].dtype == np.float32
            assert np.array_equal(a[f"records_{tag}{f}"], rec[f][idx.astype(np.int64)].astype(np.float32))
        assert np.array_equal(a["counters" + ("" if chains == 1 else "_chain1")], cnt.astype(np.float64))


def test_a_failing_rank_fails_the_bench():
    p = _run(["--gpus", "2", "--reads", "-5", "--steps", "1", "--warmup", "0"], timeout=300, script=DRY)
    assert p.returncode != 0


@pytest.mark.gpu
def test_one_gpu_through_the_plain_command():
    d = _line(_run(["--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline"]))
    assert d["n_gpus"] == 1 and d["value"] > 1000 and d["roofline"]["frac"] > 0.05
    assert "dry_run" not in d


@pytest.mark.gpu
def test_one_gpu_full_adds_the_figures_of_its_own_runs():
    d = _line(_run(["--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--full"]))
    assert d["full"] is True and d["steps"] == 5 and d["value"] > 1000
    assert d["ms_per_step_steady"] > 0 and d["ms_per_step_one_batch_in_flight"] > 0


@pytest.mark.gpu
def test_one_gpu_dump_outputs_against_the_oracle(tmp_path):
    """The plain command with --dump-outputs: the sampled records of the last timed step are the oracle's on the same reads
    (the first 3 000 of the sample, drawn again on the host from (seed, read index)), the counters are the whole step's."""
    import numpy as np
    import bench
    from decombinator_amd import _native as nat, synth
    from oracle import oracle as orc
    from tests import parity_util as pu
    d = tmp_path / "out"
    line = _line(_run(["--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d)]))
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    a = _load_dump(d)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_READS
    cnt = a["counters"]
    assert cnt[nat.COUNTER_NAMES.index("read_count")] == bench.READS_PER_GPU
    ts = synth.config_tagset(2)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    cfg = nat.synth_cfg(seed=bench.SEED, read_len=bench.READ_LEN, p_rearranged=0.45, sub_rate=0.005, n_rate=0.0005)   # (bench.py's)
    pick = idx[:3000]
    reads = [nat.unpack_reads(nat.synth_reads_host(t, cfg, int(i), 1))[0] for i in pick]
    vs, js = ts.half_splits
    ot = orc.OracleTables(ts.v_tags, ts.v_jumps, [r.upper() for r in ts.v_regions], ts.j_tags, ts.j_jumps,
                          [r.upper() for r in ts.j_regions], vs, js)
    orec, _ = pu.oracle_records(ot, reads, "reverse", False, 130)
    for f in nat.RECORD_DTYPE.names:
        assert np.array_equal(a[f"records_{f}"][:3000], orec[f].astype(np.float32)), f
    ok = (a["records_status"] == 0).mean()
    assert abs(ok - cnt[nat.COUNTER_NAMES.index("vj_count")] / bench.READS_PER_GPU) < 0.01


@pytest.mark.gpu
def test_config4_on_one_gpu_small_total():
    d = _line(_run(["--gpus", "1", "--config", "4", "--total-reads", "25000000", "--warmup", "1", "--no-cpu-baseline"]))
    assert d["scaling"] == "strong" and d["steps"] == 3 and d["value"] > 1000


def test_bench_itself_has_no_dry_switch_and_no_checker_import():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "--dry" not in src and "from tests" not in src and "import tests" not in src
    p = _run(["--gpus", "1", "--dry-gloo"], timeout=120)
    assert p.returncode != 0
