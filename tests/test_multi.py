"""The multi-GPU layer: contiguous shards, one host thread (C driver) or one process (bench.py) per GPU, and RCCL only
for the per-rank stats record (BASELINE configs[3]).

CPU part: the C shard arithmetic against glava_amd.sharding, the error behaviour without a device.
GPU part (one MI355X is all the GPU box has): the C driver glv_multi_* on a one-device "node" -- every RCCL call of the
path really executes (communicator init, all-gather, all-reduce on a communicator of size 1) -- and bench.py's own
N > 1 code path launched by torch.distributed.run with the nccl backend, with one rank and (where RCCL permits two
ranks on one device) with two.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_shard_range_matches_python(glvlib):
    from glava_amd.sharding import shard_range
    for total, world in ((524288, 8), (65536, 1), (10, 3), (7, 7), (1000003, 8), (8, 8), (9, 4)):
        covered = 0
        for rank in range(world):
            lo, cnt = glvlib.multi_shard_range(total, rank, world)
            plo, phi = shard_range(total, rank, world)
            assert (lo, lo + cnt) == (plo, phi)
            assert lo == covered
            covered += cnt
        assert covered == total


def test_multi_argument_errors(glvlib):
    G = glvlib
    p = G.Params()
    for kwargs in (dict(total_streams=8, ndev=0), dict(total_streams=8, ndev=65), dict(total_streams=1, ndev=2)):
        with pytest.raises(G.GlvError) as e:
            G.Multi(p, kwargs["total_streams"], G.OP_FFT, ndev=kwargs["ndev"])
        assert e.value.code == G.ERR_INVALID
    if G.device_count() == 0:      # the CPU-only container: no device, no CPU path
        with pytest.raises(G.GlvError) as e:
            G.Multi(p, 64, G.OP_FFT, ndev=1)
        assert e.value.code == G.ERR_NO_DEVICE


@pytest.mark.gpu
def test_c_multi_driver_on_a_one_device_node(glvlib):
    import torch
    G = glvlib
    assert torch.cuda.is_available()
    n, streams, steps = 4096, 777, 3
    p = G.Params(n=n)
    m = G.Multi(p, streams, G.OP_FFT, devices=[0])
    assert m.shard(0) == (0, 0, streams) and m.uses_rccl()
    from oracle_lib import lcg_pcm_fast
    pcm = lcg_pcm_fast(99, streams * 2 * n)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    stats, mx = m.run_s16([d_pcm], [d_out], G.OP_FFT, warmup=1, steps=steps)
    torch.cuda.synchronize()
    assert len(stats) == 1 and stats[0]["frames"] == streams * steps
    assert stats[0]["bytes"] == 12 * n * streams * steps
    assert 0 < stats[0]["seconds"] == mx and stats[0]["kernel_ms"] > 0
    # the shard's spectra are what a plain batch produces
    b = G.Batch(p, streams, G.OP_FFT)
    d_ref = torch.zeros_like(d_out)
    b.process_s16(d_pcm, d_ref, G.OP_FFT)
    torch.cuda.synchronize()
    assert torch.equal(d_out.view(torch.int32), d_ref.view(torch.int32))
    b.close(); m.close()
    # a device listed twice is refused (one shard per device)
    with pytest.raises(G.GlvError):
        G.Multi(p, 64, G.OP_FFT, devices=[0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [2, 3])
def test_c_multi_driver_several_shards_without_rccl(glvlib, monkeypatch, shards):
    """the several-shard machinery of glv_multi_run_s16 (one host thread per shard, the spin barrier around the
    timed region, per-shard streams and batches, the stats table) had only ever run with one shard.  Without RCCL
    (GLV_MULTI_RCCL=0, or a host that does not have the library) the 32-byte records are collected on the host -- the data
    path never had a collective -- and only then may one device carry several shards, which is how a one-GPU box exercises
    it: contiguous balanced shards, every shard's spectra equal to a plain batch's, every rank's table identical, the
    caller's current device restored, NULL shard pointers refused up front."""
    import torch
    G = glvlib
    monkeypatch.setenv("GLV_MULTI_RCCL", "0")
    n, streams, steps = 2048, 1001, 3
    p = G.Params(n=n)
    m = G.Multi(p, streams, G.OP_FFT, devices=[0] * shards)
    assert not m.uses_rccl()
    from oracle_lib import lcg_pcm_fast
    pcm = lcg_pcm_fast(7, streams * 2 * n).reshape(streams, 2 * n)
    b = G.Batch(p, streams, G.OP_FFT)
    d_all = torch.from_numpy(pcm).cuda()
    d_ref = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_s16(d_all, d_ref, G.OP_FFT)
    ins, outs, spans = [], [], []
    covered = 0
    for i in range(shards):
        dev, lo, cnt = m.shard(i)
        assert dev == 0 and lo == covered and cnt in (streams // shards, streams // shards + 1)
        covered += cnt
        ins.append(torch.from_numpy(np.ascontiguousarray(pcm[lo:lo + cnt])).cuda())
        outs.append(torch.zeros((cnt * 2, n), dtype=torch.float32, device="cuda"))
        spans.append((lo, cnt))
    assert covered == streams
    torch.cuda.set_device(0)
    stats, mx = m.run_s16(ins, outs, G.OP_FFT, warmup=1, steps=steps)
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == 0
    assert len(stats) == shards and [s["frames"] for s in stats] == [c * steps for _, c in spans]
    assert mx == max(s["seconds"] for s in stats) and all(s["kernel_ms"] > 0 for s in stats)
    for (lo, cnt), o in zip(spans, outs):
        assert torch.equal(o.view(torch.int32), d_ref[2 * lo:2 * (lo + cnt)].view(torch.int32)), lo
    with pytest.raises(G.GlvError) as e:
        m.run_s16([ins[0]] + [None] * (shards - 1), outs, G.OP_FFT, warmup=0, steps=1)
    assert e.value.code == G.ERR_INVALID
    b.close(); m.close()
    monkeypatch.delenv("GLV_MULTI_RCCL")
    with pytest.raises(G.GlvError):                      # with RCCL in play one device cannot carry two shards
        G.Multi(p, 64, G.OP_FFT, devices=[0, 0])


@pytest.mark.gpu
def test_eight_shards_on_eight_host_threads_do_not_serialise_on_the_host(glvlib, monkeypatch):
    """VERDICT r4 item 7 / SURVEY 8e ("anything else than linear scaling indicates host-side launch serialisation"), probed without an
    8-GPU node: glv_multi_run_s16 with EIGHT shards -- eight host threads, each with its own batch and HIP stream -- on this one device
    (host-gathered stats) against ONE shard of all the streams.  The device does the same work either way, so the eight-thread run may
    cost what eight smaller kernels per update cost (tails, less overlap) but not multiples: a lock around the launch path would
    show as ~8 x.  Every shard's spectra equal the plain batch's bit for bit."""
    import torch
    G = glvlib
    monkeypatch.setenv("GLV_MULTI_RCCL", "0")
    n, streams, steps, shards = 4096, 32768, 20, 8
    p = G.Params(n=n)
    gen = torch.Generator(device="cuda"); gen.manual_seed(8)
    d_pcm = torch.randint(-32768, 32768, (streams, n * 2), dtype=torch.int16, device="cuda", generator=gen)
    secs = {}
    for nsh in (1, shards):
        m = G.Multi(p, streams, G.OP_FFT, devices=[0] * nsh)
        ins, outs = [], []
        for i in range(nsh):
            _, lo, cnt = m.shard(i)
            ins.append(d_pcm[lo:lo + cnt]); outs.append(torch.zeros((cnt * 2, n), dtype=torch.float32, device="cuda"))
        m.run_s16(ins, outs, G.OP_FFT, warmup=20, steps=steps)
        stats, mx = m.run_s16(ins, outs, G.OP_FFT, warmup=3, steps=steps)
        torch.cuda.synchronize()
        assert len(stats) == nsh and sum(s["frames"] for s in stats) == streams * steps
        secs[nsh] = mx
        if nsh == 1: ref = outs[0].clone()
        else:
            got = torch.cat(outs)
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
        m.close()
    print(f"one shard {secs[1] / steps * 1e3:.3f} ms per update, eight shards on eight host threads {secs[shards] / steps * 1e3:.3f} ms: ratio {secs[shards] / secs[1]:.2f}")
    assert secs[shards] <= 2.5 * secs[1], secs


def _run_bench_distributed(nproc, port, extra_env=None, extra_args=()):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra_env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "3", "--warmup", "1",
           "--streams", "4096", "--no-cpu-baseline", "--no-alt", "--spinup-s", "0.05", "--sustained-s", "0", *extra_args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def _bench_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_nccl_code_path_one_rank(glvlib):
    """bench.py exactly as the driver launches it for N > 1 (torch.distributed.run, backend nccl = RCCL), with the one
    rank this box can host: init_process_group("nccl", device_id=...), barrier, all_reduce(MAX) on a device tensor and
    the all_gather of the stats record all execute on RCCL."""
    r = _run_bench_distributed(1, 29611)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _bench_line(r.stdout)
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["scaling"] == "weak"
    assert line["config"]["collectives"].startswith("nccl")


@pytest.mark.gpu
def test_bench_refuses_more_rccl_ranks_than_devices(glvlib):
    """One rank per GPU: launched with two RCCL ranks on a box with one device, bench.py refuses (non-zero exit, the reason on stderr) instead of
    letting two ranks share cuda:0 and calling it n_gpus 2.  (The functional rehearsal of the world-2 path on one device is the gloo test below.)"""
    import torch
    if torch.cuda.device_count() >= 2: pytest.skip("needs a box with a single device")
    r = _run_bench_distributed(2, 29613)
    assert r.returncode != 0
    assert "refusing to share devices" in (r.stderr + r.stdout), (r.stderr + r.stdout)[-3000:]


def _run_bench_plain(gpus, env_extra):
    env = dict(os.environ); env.update(env_extra)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"): env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "2", "--warmup", "1"],
                          capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)


def test_bench_gpus_n_without_a_launcher_spawns_n_ranks():
    """VERDICT r5 missing 5: `python bench.py --gpus 2` as a plain process (RANK unset) must not take the single-rank path.  With two devices
    visible (mocked: GLV_BENCH_DEVICE_COUNT) it runs itself under torch.distributed.run (a child process) with two ranks (the command is printed instead of
    run: GLV_BENCH_SPAWN_DRYRUN); with one device it exits non-zero and says why.  No JSON bench line in either case."""
    r = _run_bench_plain(2, {"GLV_BENCH_DEVICE_COUNT": "2", "GLV_BENCH_SPAWN_DRYRUN": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    cmd = rec["spawn"]
    assert "torch.distributed.run" in cmd and "--nproc-per-node=2" in cmd and "--nnodes=1" in cmd and "127.0.0.1" in cmd
    assert cmd[cmd.index("--gpus") + 1] == "2" and os.path.basename(cmd[cmd.index("--gpus") - 1]) == "bench.py"
    assert '"metric"' not in r.stdout
    r = _run_bench_plain(2, {"GLV_BENCH_DEVICE_COUNT": "1"})
    assert r.returncode != 0 and "only 1 HIP device(s) visible" in r.stderr and '"metric"' not in r.stdout
    r = _run_bench_plain(8, {"GLV_BENCH_DEVICE_COUNT": "0"})
    assert r.returncode != 0 and "refusing to measure fewer GPUs" in r.stderr


@pytest.mark.gpu
def test_bench_gpus_2_on_a_one_device_box_exits_non_zero(glvlib):
    """... and on the real box: `python bench.py --gpus 2` with one MI355X visible refuses instead of printing an n_gpus 1 line."""
    import torch
    if torch.cuda.device_count() >= 2: pytest.skip("needs a box with a single device")
    r = _run_bench_plain(2, {})
    assert r.returncode != 0 and "only 1 HIP device(s) visible" in r.stderr and '"metric"' not in r.stdout, (r.stderr + r.stdout)[-2000:]


@pytest.mark.gpu
def test_bench_two_ranks_with_real_kernels(glvlib, tmp_path):
    """the world > 1 path of bench.py executed with real kernels before an 8-GPU node ever sees it.  Two ranks
    share cuda:0 (RCCL refuses that, so the 32-byte stats record and the MAX all-reduce travel over gloo: GLV_BENCH_BACKEND=gloo;
    the data path has no collective either way).  Checked: both shards' stats records arrive, the line's value is the sum of the
    ranks' frames over the MAX of their seconds, rank r's shard starts at global stream r * streams, and the FIRST stream of
    every rank -- dumped by --check-dump -- is what the oracle computes for that PCM (raw FFT bit for bit, magnitudes to 1e-5)."""
    from oracle_lib import StreamOracle
    dump = str(tmp_path / "chk")
    r = _run_bench_distributed(2, 29617, {"GLV_BENCH_BACKEND": "gloo"}, ["--check-dump", dump])
    assert r.returncode == 0, (r.stderr + r.stdout)[-4000:]
    line = _bench_line(r.stdout)
    steps, streams = 3, 4096
    assert line["n_gpus"] == 2 and line["steps"] == steps and line["scaling"] == "weak"
    assert line["config"]["collectives"].startswith("gloo") and "2 rank(s)" in line["config"]["collectives"]
    stats = line["stats"]
    assert len(stats) == 2 and all(s["frames"] == streams * steps and s["kernel_ms"] > 0 and s["bytes"] == 12 * 4096 * streams * steps for s in stats)
    secs = max(s["seconds"] for s in stats)
    assert abs(line["ms_per_step"] * steps * 1e-3 - secs) < 1e-9 * max(1.0, secs) + 1e-12       # MAX over ranks
    assert abs(line["value"] - sum(s["frames"] for s in stats) / secs) <= 1e-6 * line["value"]
    pcms = []
    for rank in range(2):
        z = np.load(f"{dump}.rank{rank}.npz")
        assert int(z["rank"]) == rank and int(z["world"]) == 2 and int(z["global_stream"]) == rank * streams
        pcm = np.ascontiguousarray(z["pcm"]).reshape(-1)                       # int16 [n][2] of the rank's first stream
        want, wraw = StreamOracle(4096, gravity=False, average=False).frame(pcm, want_raw=True)
        assert (np.ascontiguousarray(z["raw"]).view(np.uint32) == np.ascontiguousarray(wraw, dtype=np.float32).view(np.uint32)).all(), rank
        assert np.allclose(z["first_spectrum"], want, rtol=1e-5, atol=0.0), rank            # magnitudes (no gravity): purely relative
        pcms.append(pcm)
    assert not (pcms[0] == pcms[1]).all()                                      # the shards hold different streams


@pytest.mark.gpu
def test_bench_line_collects_its_hbm_traffic_in_the_same_run():
    """`roofline.traffic` is collected by the bench run itself -- two separate `rocprofv3 --pmc` child passes (FETCH_SIZE, WRITE_SIZE) over the script's own
    headline launches -- and must agree with the algorithmic bytes (the pass reads every PCM byte once and writes every spectrum byte once: 1.00x) and with the committed
    measurement; with --no-live-traffic (what tools/profile.sh passes: a profiler is already wrapped around that run) the committed value is reported and says so."""
    import json
    import shutil
    if not (shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3")):
        pytest.skip("no rocprofv3 on this box")
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--no-configs", "--no-cpu-baseline", "--no-alt", "--sustained-s", "0"]
    env = {k: v for k, v in os.environ.items() if not k.startswith(("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_"))}
    r = subprocess.run(base, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    roof = json.loads(r.stdout.strip().splitlines()[-1])["roofline"]
    assert "collected in THIS run" in roof["traffic_source"], roof["traffic_live"]
    assert roof["traffic_live"]["dispatches"]["FETCH_SIZE"] >= 3 and roof["traffic_live"]["dispatches"]["WRITE_SIZE"] >= 3
    assert 0.99 < roof["traffic"] / roof["algorithmic_bytes_per_launch"] < 1.02, roof
    assert roof["traffic_committed"] is None or abs(roof["traffic"] / roof["traffic_committed"] - 1) < 0.01
    r = subprocess.run(base + ["--no-live-traffic"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    roof = json.loads(r.stdout.strip().splitlines()[-1])["roofline"]
    assert "NOT collected in this run" in roof["traffic_source"] and roof["traffic"] == roof["traffic_committed"]
