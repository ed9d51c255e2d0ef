"""bench.py's pieces that need no GPU: the live counter passes (roofline.traffic) against a stand-in profiler, and what a plain run
renders against what --full adds, with a stand-in renderer."""
import argparse
import os
import stat
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FAKE = r"""#!/bin/bash
# stands in for rocprofv3: writes the counter file the real one would, with known values
while [ $# -gt 0 ]; do case "$1" in --pmc) c=$2; shift 2;; -d) d=$2; shift 2;; --) shift; break;; *) shift;; esac; done
echo "$@" >> "$FAKE_LOG"
test -n "$FAKE_FAIL" && exit 3
mkdir -p "$d/host"
f="$d/host/1_counter_collection.csv"
echo '"Dispatch_Id","Kernel_Name","Counter_Name","Counter_Value"' > "$f"
v=100; test "$c" = WRITE_SIZE && v=40
for i in 1 2 3 4; do echo "$i,\"void trtd::k_shade<31u, true, 512, 6>(trtd::SceneDev, trtd::ShadeArgs)\",\"$c\",$v.0" >> "$f"; done
echo "5,\"void trtd::k_trace_closest<false, 1, false, 0, true, 0>(trtd::SceneDev, trtd::RaySource)\",\"$c\",10.0" >> "$f"
echo "6,\"void trtd::k_trace_closest<false, 1, false, 0, false, 0>(trtd::SceneDev, trtd::RaySource)\",\"$c\",30.0" >> "$f"
echo "7,\"void trtd::k_trace_closest<true, 1, false, 0, true, 0>(trtd::SceneDev, trtd::RaySource)\",\"$c\",999.0" >> "$f"   # the counting build: left out
echo "8,\"__amd_rocclr_copyBuffer\",\"$c\",5.0" >> "$f"
"""


def _args(**kw):
    a = dict(scene="back", width=1920, height=1080, spp=256, builder="auto", tris=None, leaf=None, seed=None, fixed_nee=False)
    a.update(kw)
    return argparse.Namespace(**a)


def _install(tmp_path, monkeypatch):
    exe = tmp_path / "rocprofv3"
    exe.write_text(FAKE)
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("PATH", f"{tmp_path}:{os.environ['PATH']}")
    monkeypatch.setenv("FAKE_LOG", str(tmp_path / "log.txt"))
    for k in [k for k in os.environ if k.startswith("ROCPROF") or k.startswith("ROCP_")]:
        monkeypatch.delenv(k)


def test_live_traffic_turns_the_counter_passes_into_bytes_per_launch(tmp_path, monkeypatch):
    """FETCH_SIZE / WRITE_SIZE are KiB summed per kernel; reads count twice (gfx950: a 128-B line is tallied as 64 B), the counting kernels of the
    untimed counting render are left out, the figure is per launch — exactly tools/pmc_summary.py's account of the committed files."""
    _install(tmp_path, monkeypatch)
    by, note = bench.live_traffic(_args(leaf=8, tris=5000))
    assert by == {"shade": (2 * 400 + 160) * 1024 // 4, "trace_closest": (2 * 40 + 40) * 1024 // 2}, (by, note)
    assert note.startswith("live:")
    log = open(tmp_path / "log.txt").read().splitlines()
    assert len(log) == 2  # one child per counter, each the program itself behind `--` (no shell, no env wrapper)
    for line in log:
        assert line.split()[0] == sys.executable and "bench.py" in line.split()[1]
        assert "--full" in line and "--no-traffic" in line and "--steps 1" in line and "--leaf 8" in line and "--tris 5000" in line


def test_live_traffic_reports_why_it_could_not_run(tmp_path, monkeypatch):
    _install(tmp_path, monkeypatch)
    monkeypatch.setenv("FAKE_FAIL", "1")
    by, note = bench.live_traffic(_args())
    assert by == {} and "failed" in note
    monkeypatch.delenv("FAKE_FAIL")
    monkeypatch.setenv("ROCPROFILER_SOMETHING", "1")   # this process is itself being profiled: no nested passes
    by, note = bench.live_traffic(_args())
    assert by == {} and "not attempted" in note


def test_dump_outputs_writes_the_image_and_ray_counts(tmp_path):
    """--dump-outputs: the whole float32 image when it fits in 64 MB, the ray counts as exact float64."""
    import numpy as np
    from tinyraytracing_amd import Stats
    img = np.random.default_rng(1).random((54, 96, 3), dtype=np.float32)
    st = Stats(rays_camera=5184, rays_shadow=7000, rays_indirect=3001)
    bench.dump_outputs(str(tmp_path / "d"), img, st)
    assert sorted(os.listdir(tmp_path / "d")) == ["image.npy", "ray_counts.npy"]
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)
    rc = np.load(tmp_path / "d" / "ray_counts.npy")
    assert rc.dtype == np.float64 and rc.tolist() == [5184, 7000, 3001]


def test_dump_outputs_samples_a_large_image_the_same_way_every_time(tmp_path):
    """An image over 64 MB (3840x2160 is 95 MB) is written as a fixed seeded sample of pixels: the same indices on every run, under 64 MB in all."""
    import numpy as np
    from tinyraytracing_amd import Stats
    img = np.arange(2160 * 3840 * 3, dtype=np.float32).reshape(2160, 3840, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img, Stats())
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["image_sample.npy", "image_sample_pixels.npy", "ray_counts.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n
    idx = np.load(tmp_path / "a" / "image_sample_pixels.npy")
    px = np.load(tmp_path / "a" / "image_sample.npy")
    assert idx.dtype == np.float64 and px.dtype == np.float32 and len(np.unique(idx)) == len(idx) == len(px)
    assert np.array_equal(px, img.reshape(-1, 3)[idx.astype(np.int64)])


def _parse(*argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_the_live_counter_passes_run_only_with_full(monkeypatch):
    """A plain run of the contract's command starts no profiler children; --full does, unless told otherwise."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert not _parse("--gpus", "1", "--steps", "3", "--warmup", "1", monkeypatch=monkeypatch).full
    assert not bench.wants_live_traffic(_parse("--gpus", "1", "--steps", "3", "--warmup", "1", monkeypatch=monkeypatch))
    assert bench.wants_live_traffic(_parse("--gpus", "1", "--full", monkeypatch=monkeypatch))
    assert not bench.wants_live_traffic(_parse("--full", "--no-traffic", monkeypatch=monkeypatch))
    assert not bench.wants_live_traffic(_parse("--full", "--scene", "veach-mis", monkeypatch=monkeypatch))
    assert bench.wants_live_traffic(_parse("--full", "--traffic", "--scene", "veach-mis", monkeypatch=monkeypatch))
    with pytest.raises(SystemExit):
        _parse("--traffic", monkeypatch=monkeypatch)


class _FakeRenderer:
    """Stands in for T.Renderer: records the flags of every render and returns fixed counts."""
    flags = []

    def __init__(self, scene, device=0):
        pass

    def render_into(self, p, out, stream):
        import tinyraytracing_amd as T
        _FakeRenderer.flags.append(p.flags)
        st = T.Stats(rays_camera=100, rays_shadow=50, rays_indirect=25, render_ms=1.0, passes=1)
        if p.flags & T.TRT_FLAG_TIMING:
            for k in range(len(T.KERNEL_NAMES)):
                st.launches[k], st.kernel_ms[k] = 2, 0.5 + k
        return st

    def close(self):
        pass


def _fake_bench(a, monkeypatch):
    """A Bench on the CPU: the real scene, params and stripe logic, a recording renderer, host tensors."""
    import types
    import torch
    import tinyraytracing_amd as T
    monkeypatch.setattr(T, "Renderer", _FakeRenderer)
    _FakeRenderer.flags = []
    B = bench.Bench(a, 1, 0, 0, None, "nccl")
    cuda = types.SimpleNamespace(current_stream=lambda: types.SimpleNamespace(cuda_stream=0), synchronize=lambda: None, empty_cache=lambda: None)
    B.torch = types.SimpleNamespace(float32=torch.float32, cuda=cuda,
                                    empty=lambda shape, dtype, device: torch.empty(shape, dtype=dtype))
    D = B.D
    B.D = types.SimpleNamespace(shard_params=D.shard_params, StepTimes=D.StepTimes,
                                render_distributed=lambda *args, device=None, **kw: D.render_distributed(*args, **kw))
    return B, T


def test_a_plain_run_renders_only_its_warmup_and_timed_steps(monkeypatch, tmp_path):
    """Without --full a workload is the counting render (the first warm-up step), the other warm-ups and the timed steps — nothing after
    them — and its line carries no figure that needs a render of its own; --dump-outputs is still written."""
    a = _parse("--steps", "3", "--warmup", "2", monkeypatch=monkeypatch)
    B, T = _fake_bench(a, monkeypatch)
    res, scene = B.measure("back", 32, 16, 4, a.steps, a.warmup, 7, also_overlap=a.full and not a.no_overlap_extra, dump_dir=str(tmp_path), full=a.full)
    assert _FakeRenderer.flags == [T.TRT_FLAG_COUNT, 0, 0, 0, 0]
    assert res["steps"] == 3 and res["warmup"] == 2 and res["rays_per_step"] == 175 and res["ms_per_step"] > 0
    for k in ("roofline", "kernels_rank0", "with_pass_overlap"):
        assert k not in res, k
    assert "kernel_ms_from" not in res["timing"]
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "ray_counts.npy"]


def test_full_adds_the_profiling_step_and_the_overlapped_steps(monkeypatch):
    a = _parse("--steps", "3", "--warmup", "2", "--full", monkeypatch=monkeypatch)
    B, T = _fake_bench(a, monkeypatch)
    res, scene = B.measure("back", 32, 16, 4, a.steps, a.warmup, 7, also_overlap=a.full and not a.no_overlap_extra, full=a.full)
    assert _FakeRenderer.flags == [T.TRT_FLAG_COUNT, 0, 0, 0, 0, T.TRT_FLAG_TIMING] + [T.TRT_FLAG_OVERLAP] * 4
    assert res["kernels_rank0"]["trace_closest"] == {"ms_per_step": 1.5, "launches_per_step": 2, "algorithmic_GBps": 0.0}
    assert res["roofline"]["kernel"] == T.KERNEL_NAMES[-1] and res["with_pass_overlap"]["unit"] == "Mrays/s"
    assert res["timing"]["kernel_ms_from"].startswith("1 profiling step")
