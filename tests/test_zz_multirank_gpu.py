"""-m gpu, LAST in a session (conftest.py orders `multirank` tests after everything else): bench.py's N > 1 launch path end to end on a one-GPU box -- two ranks
under torch.distributed.run, both on GPU 0 (--one-device moves the device ordinal only), backend gloo (RCCL refuses two ranks on one device).

Every job here runs in its own session with a hard limit; at the limit the whole process GROUP is killed and the test fails with the ranks' phase log and
stacks (bench.py prints one line per rank and phase and dumps every rank's stack periodically), so a stall names the call it stalled in."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

pa = ol.pa
ROOT = ol.ROOT
pytestmark = [pytest.mark.gpu, pytest.mark.multirank, pytest.mark.timeout(1500)]

BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--steps", "1", "--warmup", "1", "--tris", "200000", "--res", "320", "192", "--spp", "4", "--cpu-seconds", "0", "--traffic", "none"]
SCENE_KEY = "sanmiguel_synth_200k_320x192_4spp"


def _end(p, limit_s):
    """wait for p (leader of its own process group) up to limit_s; then SIGTERM (bench.py's launcher ends its ranks), SIGKILL after 20 s.  rc or None = stopped at the limit"""
    try:
        return p.wait(timeout=limit_s)
    except subprocess.TimeoutExpired:
        for sig, grace in ((signal.SIGTERM, 20), (signal.SIGKILL, 10)):
            try:
                os.killpg(p.pid, sig)
            except (ProcessLookupError, PermissionError):
                pass
            try:
                p.wait(timeout=grace)
                break
            except subprocess.TimeoutExpired:
                pass
        return None
    finally:
        try:
            os.killpg(p.pid, signal.SIGKILL)   # whatever is left of the group (the ranks end with their launcher: parallel.die_with_parent)
        except (ProcessLookupError, PermissionError):
            pass


@pytest.fixture(scope="module", autouse=True)
def torch_is_warm():
    """The first `import torch` + first device tensor on a fresh box page in gigabytes of the image and have taken anything from one to ten minutes (the stall of
    round 5's driver run, reproduced in round 6: profiles/r06_a_*).  conftest.py starts that warm-up in the background when the session begins; here it is
    awaited (bounded) BEFORE any job's own limit starts to count, so the limits below measure the jobs, not the box."""
    import time
    import conftest
    t0 = time.time()
    w = getattr(conftest, "TORCH_WARMUP", None)
    if w is None:
        w = subprocess.Popen([sys.executable, "-c", conftest.TORCH_WARMUP_CODE], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
    rc = _end(w, 480)   # (the session's limit on the driver's box is 1200 s for the whole suite: 480 s here + the warm-up's head start of the two hundred tests before it)
    print("[multirank] torch warm-up: rc %s, waited %.0f s" % (rc, time.time() - t0))
    yield


def run_job(args, tmp_path, limit_s=300, extra_env=None):
    """`python bench.py args` in its own process group, stderr to a file; (rc, stdout, stderr) -- rc None = stopped at the limit"""
    import time
    env = dict(os.environ, PBRT_AMD_BENCH_DIR=str(tmp_path), PBRT_AMD_BENCH_STACKS_S="60", PBRT_AMD_BENCH_WAIT_S="180", PBRT_AMD_PG_TIMEOUT_S="180")
    env.update(extra_env or {})
    err_path, out_path = str(tmp_path / "job.err"), str(tmp_path / "job.out")
    t0 = time.time()
    with open(err_path, "w") as ferr, open(out_path, "w") as fout:
        p = subprocess.Popen([sys.executable, BENCH] + args, stdout=fout, stderr=ferr, env=env, start_new_session=True)
        rc = _end(p, limit_s)
    print("[multirank] bench.py %s: rc %s after %.0f s" % (" ".join(args[:4]), rc, time.time() - t0))
    return rc, open(out_path).read(), open(err_path).read()


def test_bench_two_ranks_self_launch_end_to_end(tmp_path):
    """`python bench.py --gpus 2` starts its own two ranks (one process per GPU), local rank 0 generates the scene, builds it and publishes the blob, rank 1 MAPS
    it; the tiles are sharded, rank 1's reachable FilmTilePixels are added into rank 0's film, ONE JSON line for the whole job.  Checked: the line; the
    whole-job sample count (every pixel exactly once across the ranks); how each rank got its scene; and the IMAGE -- rank 0's combined film equals the
    one-process render of the same scene file, bit for bit on the pixels that only hold their own samples (film.cpp:117-130: a merge of disjoint tiles)."""
    film2 = str(tmp_path / "film2.npy")
    rc, out, err = run_job(["--gpus", "2", "--one-device", "--backend", "gloo", "--dump-film", film2] + SMALL, tmp_path)
    assert rc == 0, "rc %s (None = killed at the limit)\n%s" % (rc, err[-6000:])
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "strong" and d["unit"] == "Msamples/s"
    assert abs(d["value"] * 1e6 * d["ms_per_step"] * 1e-3 - 320 * 192 * 4) <= 0.01 * 320 * 192 * 4   # all samples of the frame, once
    assert d["setup_s"]["scene_by_rank"] == ["built", "mapped"], d["setup_s"]
    assert len([l for l in err.splitlines() if l.startswith("wrote ") and "sanmiguel_synth.pbrt" in l]) == 1, "the scene was generated %d times" % err.count("wrote ")
    # the image: one process, one context, the same file
    got = np.load(film2)
    sc = pa.Scene(os.path.join(str(tmp_path), SCENE_KEY, "sanmiguel_synth.pbrt"), strict=True)
    ctx = pa.Context(sc)
    ctx.render()
    ref = ctx.film()
    ctx.close()
    assert got.shape == ref.shape == (192, 320, 4)
    own_only = ref[..., 3] == sc.info["spp"]
    assert own_only.mean() > 0.98
    assert np.array_equal(got[own_only].view(np.uint32), ref[own_only].view(np.uint32))
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-7)
    assert np.array_equal(got[..., 3] != 0, ref[..., 3] != 0)
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("pbrt_amd_scene_") and ("%d" % os.getpid()) in f]   # the blob is gone


def test_bench_one_rank_film_equals_the_library_render(tmp_path):
    """the N = 1 line of the same command dumps the same film the library renders in-process (the dump is what the 2-rank test compares)"""
    film1 = str(tmp_path / "film1.npy")
    rc, out, err = run_job(["--gpus", "1", "--dump-film", film1, "--secondary", "off"] + SMALL, tmp_path)
    assert rc == 0, err[-3000:]
    sc = pa.Scene(os.path.join(str(tmp_path), SCENE_KEY, "sanmiguel_synth.pbrt"), strict=True)
    ctx = pa.Context(sc)
    ctx.render()
    own_only = ctx.film()[..., 3] == sc.info["spp"]
    assert np.array_equal(np.load(film1)[own_only].view(np.uint32), ctx.film()[own_only].view(np.uint32))
    ctx.close()


def test_bench_plain_line_times_the_steps_and_dumps_the_film(tmp_path):
    """a plain run (no --full): exactly --steps timed steps, the headline fields and no more, and --dump-outputs writes the last timed step's film -- the film
    the library renders in-process for the same scene file"""
    out_dir = tmp_path / "outputs"
    rc, out, err = run_job(["--gpus", "1", "--dump-outputs", str(out_dir)] + SMALL + ["--steps", "3"], tmp_path)
    assert rc == 0, err[-3000:]
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-500:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] * 1e6 * d["ms_per_step"] * 1e-3 - 320 * 192 * 4) <= 0.01 * 320 * 192 * 4   # one step = every sample of the frame once
    assert not {"roofline", "roofline_shade", "cpu_baseline", "secondary"} & set(d), sorted(d)
    assert sorted(os.listdir(out_dir)) == ["film.npy"]
    got = np.load(out_dir / "film.npy")
    assert got.dtype == np.float32
    sc = pa.Scene(os.path.join(str(tmp_path), SCENE_KEY, "sanmiguel_synth.pbrt"), strict=True)
    ctx = pa.Context(sc)
    ctx.render()
    ref = ctx.film()
    ctx.close()
    assert got.shape == ref.shape == (192, 320, 4)
    own_only = ref[..., 3] == sc.info["spp"]
    assert np.array_equal(got[own_only].view(np.uint32), ref[own_only].view(np.uint32))


def test_bench_full_keeps_the_roofline(tmp_path):
    """--full still measures what moved out of the plain run: the counting pass behind the roofline's per-ray figures and the stream / gather ceilings"""
    rc, out, err = run_job(["--gpus", "1", "--full", "--secondary", "off"] + SMALL, tmp_path)
    assert rc == 0, err[-3000:]
    d = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    r = d["roofline"]
    assert r["nodes_per_ray"] > 1 and r["tris_per_ray"] > 0 and r["hbm_stream_read_GBps"] > 0 and r["request_rate"]["ceilings_Greq_per_s"]["L2_2MB"] > 0
    assert "cpu_baseline" in d and d["cpu_baseline"] is None   # --cpu-seconds 0


def test_a_cut_off_scene_file_fails_both_ranks_loudly(tmp_path):
    """A PLY file shorter than its header promises (cut off, or caught half-written) is an ERROR on the rank that reads it -- never a smaller scene: local rank 0
    fails its strict load and announces why, rank 1 stops waiting and fails with that reason (or is ended by the launcher first), the job ends non-zero well
    inside the limit and prints no line."""
    d = tmp_path / SCENE_KEY
    d.mkdir()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_scenes.py"), "sanmiguel", "--tris", "200000", "--res", "320", "192", "--spp", "4",
                           "--out", str(d / "sanmiguel_synth.pbrt")], stdout=subprocess.DEVNULL)
    ply = d / "sanmiguel_synth_geo" / "m03.ply"
    size = ply.stat().st_size
    with open(ply, "r+b") as f:
        f.truncate(size - size // 3)
    (d / ".done").write_text("ok")
    rc, out, err = run_job(["--gpus", "2", "--one-device", "--backend", "gloo"] + SMALL, tmp_path, limit_s=240)
    assert rc is not None and rc != 0, "rc %s\n%s" % (rc, err[-3000:])
    assert not [l for l in out.splitlines() if l.startswith("{")]
    assert "Unable to read the contents of PLY file" in err and "strict mode" in err, err[-3000:]
    assert "Traceback" in err and "timed out" not in err
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("pbrt_amd_scene_") and f.endswith(".failed")], "the failed job left its note behind"


def _run_script(code, tmp_path, limit_s=240):
    """python -c code in its own process group with a hard limit; (rc, stdout + stderr) -- rc None = killed at the limit"""
    out_path = str(tmp_path / "script.out")
    env = dict(os.environ, PYTHONFAULTHANDLER="1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    with open(out_path, "w") as fout:
        p = subprocess.Popen([sys.executable, "-c", code], stdout=fout, stderr=subprocess.STDOUT, env=env, start_new_session=True, cwd=ROOT)
        rc = _end(p, limit_s)
    return rc, open(out_path).read()


def test_the_librarys_rccl_step_executes_on_this_gpu(tmp_path):
    """mi_film_gather's distinct-device branch cannot run on a one-GPU box (RCCL refuses two ranks on one device).  mi_rccl_probe runs the pieces it is made of on
    the one GPU there is: librccl.so loaded with dlopen, ncclCommInitAll over {device 0}, ONE ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd of packed
    FilmTilePixels on the context's stream (the helper the gather itself calls), the gather's add kernel; every pixel must arrive bit for bit."""
    code = ("import importlib, os, sys; sys.path.insert(0, %r); pa = importlib.import_module('pbrt-v3-distributed_amd'); "
            "sc = pa.Scene(os.path.join(%r, 'scenes', 'cornell.pbrt')); ctx = pa.Context(sc); ctx.rccl_probe(1 << 16); ctx.rccl_probe(1000003); ctx.close(); print('RCCL_PROBE_OK')" % (ROOT, ROOT))
    rc, out = _run_script(code, tmp_path)
    assert rc == 0 and "RCCL_PROBE_OK" in out, "rc %s\n%s" % (rc, out[-3000:])


def test_sharded_frame_over_rccl_with_one_rank(tmp_path):
    """parallel.ShardedFrame / FilmExchange on backend "nccl" (= RCCL) with a world of ONE rank on the real GPU: init_process_group with the device id, the film
    tensors, the all-reduces of max_over_ranks / sum_over_ranks, the barriers of sync_all and a grouped batch_isend_irecv of packed pixels to itself all
    execute RCCL code on hardware (the N > 1 collectives differ in peers, not in calls); the exchanged frame equals the plain render bit for bit."""
    code = """
import importlib, os, sys
import numpy as np
sys.path.insert(0, %r)
pa = importlib.import_module('pbrt-v3-distributed_amd'); par = importlib.import_module('pbrt-v3-distributed_amd.parallel')
import torch, torch.distributed as dist
sc = pa.Scene(os.path.join(%r, 'scenes', 'cornell.pbrt'))
ctx = pa.Context(sc); ctx.render(); ref = ctx.film()
torch.cuda.set_device(0)
import datetime
dist.init_process_group(backend='nccl', device_id=torch.device('cuda', 0), timeout=datetime.timedelta(seconds=120))
# the collectives ShardedFrame issues with N > 1, on the one-rank communicator
t = torch.tensor([1.5, 2.5], dtype=torch.float64, device='cuda'); dist.all_reduce(t, op=dist.ReduceOp.MAX); dist.all_reduce(t, op=dist.ReduceOp.SUM)
assert t.cpu().tolist() == [1.5, 2.5]
dist.barrier(); torch.cuda.synchronize()
# FilmExchange's grouped point-to-point exchange, rank 0 to itself: pack -> one batch_isend_irecv group -> index_add
film = torch.from_numpy(ref.reshape(-1)).cuda()
idx = torch.from_numpy(par.reach_pixels(0, 1, sc.width, sc.height, sc.info['sample_bounds'], (sc.info['crop_x0'], sc.info['crop_y0']), sc.info['filter_radius'])).cuda()
packed = film.view(-1, 4).index_select(0, idx); recv = torch.empty_like(packed)
for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, packed, 0), dist.P2POp(dist.irecv, recv, 0)]):
    w.wait()
acc = torch.zeros_like(film); acc.view(-1, 4).index_add_(0, idx, recv); torch.cuda.synchronize()
assert np.array_equal(acc.cpu().numpy().view(np.uint32), ref.reshape(-1).view(np.uint32))
obj = [None]; dist.all_gather_object(obj, 'built'); assert obj == ['built']
dist.barrier(); dist.destroy_process_group(); ctx.close()
print('RCCL_ONE_RANK_OK')
""" % (ROOT, ROOT)
    rc, out = _run_script(code, tmp_path)
    assert rc == 0 and "RCCL_ONE_RANK_OK" in out, "rc %s\n%s" % (rc, out[-3000:])
