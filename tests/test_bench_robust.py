"""bench.py's N > 1 flow cannot lose its headline: the steps after the timed
frames -- the frame-end gather, its check and the other split -- run guarded, every collective has
a timeout (MCPT_DIST_TIMEOUT_S), and rank 0 prints the JSON line with the failure in
gather.error / <split>.error.  Two gloo ranks on the CPU run bench.main() end to end with a
stand-in tracer (the allocation rules of runtime.cpp, tests/test_dist.py::_FakeTracer); the gather
is the real point-to-point transport of mcpt/parallel.py, and one rank is made to fail in it.
Those steps belong to --full; a plain run (one rank, the same stand-in tracer) renders its warmup and
timed frames only, and --dump-outputs writes the last timed frame's film."""
import contextlib
import io
import json
import os
import socket
import types

import torch.multiprocessing as mp

from test_dist import _FakeTracer


class _Tracer(_FakeTracer):
    device_name = "fake (CPU)"

    def set_work_counters(self, on=True):
        pass

    def trace_profile(self, reset=True):
        return None

    def hbm_copy_gbps(self, *a, **kw):
        return 0.0

    def close(self):
        pass


def _fake_torch():
    import torch

    cuda = types.SimpleNamespace(synchronize=lambda: None, set_device=lambda d: None, device_count=lambda: 1)
    return types.SimpleNamespace(cuda=cuda, tensor=torch.tensor, zeros_like=torch.zeros_like, float64=torch.float64,
                                 float32=torch.float32, device=torch.device, empty=torch.empty)


def _worker(rank, world, port, fail_rank, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank), MCPT_BENCH_BACKEND="gloo", MCPT_DIST_TIMEOUT_S="8")
    import torch

    import bench
    from mcpt import parallel

    def gather_film_to_root(pt, rank, world, tile=256):
        if rank == fail_rank:
            raise RuntimeError("injected gather failure")
        n = len(parallel.tiles_for_rank(rank, world, pt.W, pt.H, tile)) * tile * tile
        import torch.distributed as dist

        return parallel.gather_packed_to_root(torch.zeros((n, 4)), rank, world, dist, pt.W, pt.H, tile)

    parallel.gather_film_to_root = gather_film_to_root
    out = io.StringIO()
    err = None
    try:
        with contextlib.redirect_stdout(out):
            bench.main(["--gpus", str(world), "--full", "--steps", "1", "--warmup", "0", "--no-verify-gather",
                        "--no-work-counters"], tracer=lambda *a: (_Tracer(), None, None), torch_mod=_fake_torch())
    except BaseException as e:  # noqa: BLE001
        import traceback

        err = traceback.format_exc()
    q.put((rank, out.getvalue(), err))


def _run(world, fail_rank):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fail_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, text, err = q.get(timeout=180)
        res[r] = (text, err)
    for p in procs:
        p.join(60)
    return res


def test_gather_failure_still_prints_the_headline_gloo_world2():
    res = _run(2, fail_rank=1)
    text, err = res[0]
    assert err is None and res[1][1] is None
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 prints one JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "error" in d["gather"]  # rank 0 timed out in its receive, or saw rank 1's failure
    assert d["weak"]["error"].startswith("skipped")  # the other split is not attempted after a failure
    assert d["config"]["product"] is False and "MCPT_BENCH_BACKEND" in d["config"]["knobs"]
    assert res[1][0] == ""  # only rank 0 prints


class _PlainTracer(_Tracer):
    """A plain run ends with its timed frames: nothing that --full owns may be asked of the tracer."""
    frames = 0

    def render(self):
        self.frames += 1
        return super().render()

    def film(self):
        import numpy as np

        Ld = np.arange(self.H * self.W * 3, dtype=np.float32).reshape(self.H, self.W, 3) + self.frames
        return Ld, np.full((self.H, self.W), self.frames, np.uint32)

    def set_work_counters(self, on=True):
        raise AssertionError("counting frame in a plain run")

    def hbm_copy_gbps(self, *a, **kw):
        raise AssertionError("copy ceiling measured in a plain run")


def test_plain_run_times_its_steps_and_dumps_the_last_frame(tmp_path, monkeypatch, capsys):
    import numpy as np

    import bench

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("CPU baseline")))
    pt = _PlainTracer()
    bench.main(["--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "d")],
               tracer=lambda *a: (pt, None, None), torch_mod=_fake_torch())
    d = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][0])
    assert pt.frames == 5 and d["steps"] == 3 and d["warmup"] == 2  # --steps sets the timed frames, nothing after them
    assert d["ms_per_step"] >= 2.0 and d["full"] is False and d["roofline"] is None and d["cpu_baseline"] is None
    assert {"metric", "value", "unit", "higher_is_better", "dtype"} <= set(d)
    Ld, smp = np.load(tmp_path / "d" / "film_Ld.npy"), np.load(tmp_path / "d" / "film_samples.npy")
    assert Ld.dtype == np.float32 and smp.dtype == np.float32 and Ld.shape == (1080, 1920, 3)
    assert np.all(smp == 5) and Ld[0, 0, 0] == 5  # the film of the last timed frame


def test_dump_outputs_samples_a_large_film_the_same_way_every_run(tmp_path, monkeypatch):
    import numpy as np

    import bench

    pt = _PlainTracer()
    pt.W, pt.H = 64, 48
    monkeypatch.setattr(bench, "DUMP_BYTES", 24 * 1000)  # 64 x 48 x 16 B does not fit: 1000 pixels at 24 B
    bench.dump_outputs(pt, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(pt, str(tmp_path / "b"), 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["film_Ld.npy", "film_pixels.npy", "film_samples.npy"]
    a = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(np.array_equal(a[f], np.load(tmp_path / "b" / f)) for f in files)
    assert sum(v.nbytes for v in a.values()) <= 24 * 1000
    px = a["film_pixels.npy"].astype(np.int64)
    assert len(np.unique(px)) == 1000 and px.min() >= 0 and px.max() < 64 * 48
    assert np.array_equal(a["film_Ld.npy"], pt.film()[0].reshape(-1, 3)[px])
    # N > 1: every rank writes its own files within its share
    bench.dump_outputs(pt, str(tmp_path / "c"), 1, 2)
    assert sorted(os.listdir(tmp_path / "c")) == ["film_Ld_rank1.npy", "film_pixels_rank1.npy", "film_samples_rank1.npy"]
    assert len(np.load(tmp_path / "c" / "film_pixels_rank1.npy")) == 500


def test_gather_success_gloo_world2():
    res = _run(2, fail_rank=-1)
    d = json.loads([ln for ln in res[0][0].splitlines() if ln.startswith("{")][0])
    assert "error" not in d["gather"] and d["gather"]["gather_backend"] == "gloo"
    assert "error" not in d["weak"] and d["weak"]["frame"] == [1920, 2160]
