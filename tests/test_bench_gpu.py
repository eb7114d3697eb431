"""bench.py's N-rank flow, run as the driver runs it.  A file of its own, first in the session: its children are the only processes on the GPU then."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_runs_its_two_rank_flow_on_one_gpu():
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one process per rank), with both ranks on THIS box's one GPU (--shared-gpu: gloo for the process
    group, the peer-write composer between the processes): the N-rank control flow of the file -- both legs' frames, the balancing rounds with their all-gathers,
    brmi_set_band / brmi_compose_set_bounds, composition of every frame, the max-over-ranks reduction, rank 0's ONE line -- runs end to end and the line has the
    contract's fields.  Its numbers are two processes sharing a GPU; nothing is asserted about them beyond being there."""
    import json
    import socket
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BRMI_BENCH_PEER_TIMEOUT_MS="10000")
    # Two processes' device-side waits for each other need both processes' queues ON the one GPU at the same time; when the scheduler time-slices them instead (seen once
    # in a session whose parent process held queues of 200 earlier tests) a wait runs into its timeout and bench.py refuses the run -- an artefact of sharing the GPU,
    # so the check is repeated rather than failed on that one message.
    for attempt in range(3):
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.join(ROOT, "bench.py"), "--gpus", "2", "--shared-gpu", "--full", "--steps", "4", "--warmup", "3", "--balance-rounds", "2", "--balance-frames", "6"]
        done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        text = done.stdout.decode(errors="replace")
        if done.returncode == 0 or "a wait for a peer's band" not in text:
            break
    assert done.returncode == 0, text[-4000:]
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, text[-4000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["warmup"] == 3 and out["higher_is_better"] is True and out["scaling"] == "weak"
    assert out["metric"].startswith("shaded Mpixels/s") and out["unit"] == "Mpixels/s" and out["value"] > 0 and out["ms_per_step"] > 0
    assert "shared_gpu" in out
    assert out["config"]["baseline_config"].startswith("configs[2]")      # the line's own value: the headline scene, weak-scaled
    for leg in ("weak", "configs3_weak", "configs3_strong"):
        assert out[leg]["rank_ms_per_step"]["ranks"] == 2 and out[leg]["value"] > 0 and out[leg]["n1_reference"]["value"] > 0 and 0 < out[leg]["efficiency_vs_n1"]
    assert out["config"]["partition"].startswith("cost-balanced contiguous bands")


@pytest.mark.gpu
def test_bench_falls_back_to_peer_writes_when_rccl_refuses():
    """The RCCL composer of the N-GPU bench has never had more than one rank on this pool.  Should it fail on the driver's node, every rank must learn so together and the run
    must go on: here RCCL does refuse (two ranks on ONE device: 'Duplicate GPU detected'), the ranks agree, the peer-write composer takes over, and the line says what happened."""
    import json
    import socket
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BRMI_BENCH_PEER_TIMEOUT_MS="10000", BRMI_BENCH_KEEP_COMPOSER="1")
    for attempt in range(3):
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.join(ROOT, "bench.py"), "--gpus", "2", "--shared-gpu", "--workload", "sponza", "--legs", "weak", "--steps", "3", "--warmup", "2", "--balance-rounds", "1", "--balance-frames", "4"]
        done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        text = done.stdout.decode(errors="replace")
        if done.returncode == 0 or "a wait for a peer's band" not in text:
            break
    assert done.returncode == 0, text[-4000:]
    out = json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["value"] > 0
    assert "native composer failed" in out["config"]["workload"] and "peer" in out["config"]["workload"], out["config"]["workload"]


@pytest.mark.gpu
def test_plain_bench_times_its_steps_once_and_dumps_the_same_outputs_twice(tmp_path):
    """bench.py --gpus 1 as the driver runs it, twice with --dump-outputs: ONE line with the headline's fields, --steps frames timed in one region and nothing
    of --full (no roofline, stage profile, camera paths, CPU baselines or other workloads); the last step's outputs as float32 / float64 .npy files under
    64 MB, the same arrays in both runs."""
    import json
    import subprocess
    import sys
    import numpy as np
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d)]
        done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        text = done.stdout.decode(errors="replace")
        assert done.returncode == 0, text[-4000:]
        lines = [ln for ln in text.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, text[-4000:]
        out = json.loads(lines[0])
        assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 2 and out["repeats"] == 1
        assert out["metric"].startswith("shaded Mpixels/s") and out["unit"] == "Mpixels/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert out["value"] > 0 and out["ms_per_step"] > 0 and out["ms_per_step_minmax"] == [out["ms_per_step"]] * 2
        assert not {"roofline", "stage_ms", "serial_frame_ms", "path", "path_fast", "cpu_baseline", "configs0", "configs1", "configs3", "configs4", "dense", "skinned"} & set(out)
        names = sorted(os.listdir(d))
        assert names == ["counters.npy", "depth.npy", "hdr.npy", "visibility.npy"]
        assert sum(os.path.getsize(d / n) for n in names) < 64 << 20
        arrays = {n[: -len(".npy")]: np.load(d / n) for n in names}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["hdr"].shape == (1 << 20, 4) and arrays["depth"].shape == (1 << 20,) and arrays["visibility"].shape == (1 << 20, 2)
        assert arrays["counters"][0] > 0 and (arrays["visibility"][:, 0] != 0xFFFFFFFF).any()      # something was drawn
        dumps.append(arrays)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n], equal_nan=True), n


def _ring_frame_of_last_step(passes, warmup, steps):
    """Index, in the chain of frames each one tested phase 1 against, of the frame bench.measure dumps (its last timed step): the passes of the ring render
    frames in turn and pass k reads the chain of pass k - 1; the warm-up and the timed region each start at pass 0, so the first timed frame reads the
    chain of the warm-up's frame on the ring's last pass, not of the warm-up's last frame.  A pass whose source has rendered nothing yet tests nothing
    (frame 0 of the chain)."""
    last = [-1] * passes

    def frame(k):
        last[k] = last[(k - 1) % passes] + 1

    for f in range(warmup):
        frame(f % passes)
    for s in range(steps):
        frame(s % passes)
    return last[(steps - 1) % passes]


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["bistro", "san_miguel", "zorah"])
def test_bench_dumped_frame_matches_the_oracle(workload, tmp_path):
    """The frame the bench times, from the bench process itself: `bench.py --gpus 1 --workload W --steps 20 --warmup 5 --dump-outputs` (three passes in a ring,
    the geometry stream and the shading streams, no host wait between frames, default tuning: the draw list, the lean rasteriser, the direct walks and the wide
    pass decided from feedback words a frame or two old) against the oracle's frame at the same place of the chain.  The headline scene, the alpha-tested
    San-Miguel-class frame and the Zorah-class 8K frame (lean rasteriser, half of its clusters held back).  At the dumped pixels: both visibility words and
    depth exact, HDR within one fp16 ULP where the oracle drew something; the visible-cluster counts of both phases and the meshlets tested exact."""
    import subprocess
    import sys
    import numpy as np
    import bench
    import orc
    from basicrenderer_amd import Scene, compose
    steps, warmup = 20, 5
    d = tmp_path / workload
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)]
    done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = done.stdout.decode(errors="replace")
    assert done.returncode == 0, text[-4000:]
    got = {n: np.load(d / (n + ".npy")) for n in ("hdr", "depth", "visibility", "counters")}

    preset, kw, features = bench.WORKLOADS[workload]
    W, H = bench.FRAME_SIZE.get(workload) or compose.frame_size(1, "stripes")
    sc = Scene(preset, W, H, point_lights=bench.LIGHTS[workload], directional=True, material_features=features, **kw)
    o = orc.OracleFrame(sc)
    # A still camera: a frame is a function of the chain it tests phase 1 against, so the chain stops changing once it returns what it was given
    last = _ring_frame_of_last_step(3, warmup, steps)
    hz = None
    for k in range(last + 1):
        given = hz
        hz = o.run_occlusion(given)
        if given is not None and np.array_equal(hz[0], given[0]):
            break
    o.gbuffer(); o.light_cluster(); o.shade()
    print(f"[bench dump] {workload}: the oracle's chain settled at frame {k} of {last}; visible clusters {o.count1} + {o.count2}")

    px = np.sort(np.random.default_rng(0).choice(H * W, size=min(H * W, bench.DUMP_PIXELS), replace=False))
    vis = o.vis.reshape(-1)[px]
    assert got["visibility"].shape == (len(px), 2)
    hi, lo = got["visibility"][:, 0].astype(np.uint64), got["visibility"][:, 1].astype(np.uint64)
    assert np.array_equal(hi, vis >> np.uint64(32)) and np.array_equal(lo, vis & np.uint64(0xFFFFFFFF)), \
        f"{int(((hi << np.uint64(32)) | lo != vis).sum())} of {len(px)} sampled keys differ from the oracle's"
    assert np.array_equal(got["depth"].astype(np.float32).view(np.uint32), o.depth.reshape(-1)[px].view(np.uint32)), "linear depth"
    covered = vis != np.uint64(0xFFFFFFFFFFFFFFFF)
    assert covered.any()
    a = got["hdr"].astype(np.float16).view(np.uint16).astype(np.int32)[covered]
    b = o.hdr.reshape(-1)[px].view(np.uint16).reshape(-1, 4).astype(np.int32)[covered]
    assert np.abs(a - b).max() <= 1, f"HDR differs by up to {int(np.abs(a - b).max())} fp16 ULP"
    want = [o.count1, o.count2, o.counters.meshletsTested + o.counters2.meshletsTested]
    assert got["counters"].astype(np.int64).tolist() == want, (got["counters"].tolist(), want)
