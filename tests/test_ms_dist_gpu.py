"""Multi-GPU product path on the GPU box: video-stitcher_amd/stitch_dist (one thread per rank over ms_dist) must deliver, on the sink, the SAME
I420 frames whatever the number of ranks, the batch size, the column-shard grouping and the transport -- compared through `checksum_all` with
the single-rank run.  With one GPU on the box the ranks share it over the host (shared-memory) transport; where two or more GPUs are visible
the same tests also run over RCCL.  The single-rank runs already go through RCCL (a communicator of one), so the library is loaded, the
communicator initialised and its all-gather executed on every box."""
import json
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import synth
from helpers import make_rig, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_dist")


_REF_RUNS = {}      # single-rank reference runs are pure functions of their arguments: a dozen tests ask for the same ones


def run(*args, rig="mini6", timeout=600, env=None):
    key = (tuple(str(a) for a in args), rig)
    if env is None and len(args) >= 2 and str(args[0]) == "--gpus" and str(args[1]) == "1":
        if key not in _REF_RUNS:
            _REF_RUNS[key] = _run(*args, rig=rig, timeout=timeout, env=None)
        return _REF_RUNS[key]
    return _run(*args, rig=rig, timeout=timeout, env=env)


def _run(*args, rig="mini6", timeout=600, env=None):
    cfg = synth.CONFIGS[rig]
    base = ["--views", cfg["n"], "--size", "%dx%d" % (cfg["w"], cfg["h"]), "--out", "%dx%d" % (cfg["out_w"], cfg["out_h"]), "--hfov", cfg["hfov_deg"], "--bands", cfg["num_bands"]]
    out = subprocess.run([APP] + [str(a) for a in base + list(args)], capture_output=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    return json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])


def multi(n):
    """arguments that put n ranks on this box: their own GPUs over RCCL if there are enough, else all on device 0 over the host transport"""
    return ["--gpus", n] if torch.cuda.device_count() >= n else ["--gpus", n, "--share-gpu"]


def test_single_rank_runs_over_rccl_and_matches_the_python_binding(ms, cuda):
    one = run("--gpus", 1, "--frames", 8, "--batch", 4)
    assert one["dist"]["transport"] == "rccl" and one["dist"]["nranks"] == 1 and one["dist"]["comm_nranks"] == 1 and one["dist"]["rccl_version"] > 0
    assert one["frames"] == 8 and len(one["dist"]["pci_bus_ids"][0]) > 4
    # frame 0 of the app = synth pattern variant 0: the same frame through the binding's ms_stitch_i420
    cfg = synth.CONFIGS["mini6"]
    comp, _, _ = make_rig(ms, "mini6")
    frames = [to_dev(synth.frame(cfg["w"], cfg["h"], i, 0, noise=False)) for i in range(cfg["n"])]
    slab = comp.new_i420(1)
    comp.stitch_i420([frames], slab)
    torch.cuda.synchronize()
    h = 1469598103934665603
    for b in slab[0].cpu().numpy().tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert "%016x" % h == one["first_frame_checksum"]
    comp.close()


@pytest.mark.parametrize("ranks,batch", [(2, 2), (2, 4), (4, 1)])
def test_frame_parallel_ranks_deliver_the_single_gpu_frames(cuda, ranks, batch):
    one = run("--gpus", 1, "--frames", 16, "--batch", 4)
    many = run(*multi(ranks), "--frames", 16, "--batch", batch)
    assert many["dist"]["nranks"] == ranks and many["frames"] == 16
    assert many["checksum_all"] == one["checksum_all"]
    if torch.cuda.device_count() >= ranks:
        assert many["dist"]["transport"] == "rccl" and many["dist"]["comm_nranks"] == ranks and len(set(many["dist"]["pci_bus_ids"])) == ranks
    else:
        assert many["dist"]["transport"] == "host" and many["share_gpu"] is True


def test_tables_blob_broadcast_from_rank_0(cuda):
    """--tables-from-rank0: only rank 0 calibrates; ms_save_tables -> ms_dist_broadcast -> ms_load_tables gives every other rank bit-identical tables (timed.cpp:553
    re-runs stitch_calib at every start of every process): the frames on the sink equal those of ranks that calibrated themselves."""
    one = run("--gpus", 1, "--frames", 16, "--batch", 4)
    assert run("--gpus", 1, "--frames", 16, "--batch", 4, "--tables-from-rank0")["checksum_all"] == one["checksum_all"]
    for ranks in (2, 4):
        assert run(*multi(ranks), "--frames", 16, "--batch", 2, "--tables-from-rank0")["checksum_all"] == one["checksum_all"], ranks
    cp = run("--gpus", 1, "--frames", 16, "--batch", 4, "--recalib-every", 8)
    assert run(*multi(2), "--frames", 16, "--batch", 4, "--recalib-every", 8, "--tables-from-rank0")["checksum_all"] == cp["checksum_all"]


def test_recalibration_broadcast_swaps_meshes_at_the_agreed_frame(cuda):
    """cfg3 shape: CPW on, new meshes every 8 frames from rank 0's recalibration thread, broadcast one batch ahead with the swap frame."""
    one = run("--gpus", 1, "--frames", 32, "--batch", 4, "--recalib-every", 8, "--mesh", "9x11")
    assert one["recalibrations_applied"] == 3 and one["cpw"] is True
    static = run("--gpus", 1, "--frames", 32, "--batch", 4, "--cpw", "--mesh", "9x11")
    assert static["checksum_all"] != one["checksum_all"], "the recalibrations must change the frames"
    assert static["first_frame_checksum"] == one["first_frame_checksum"]
    for ranks, batch in ((2, 4), (2, 2), (4, 2)):
        many = run(*multi(ranks), "--frames", 32, "--batch", batch, "--recalib-every", 8, "--mesh", "9x11")
        assert many["recalibrations_applied"] == 3
        assert many["checksum_all"] == one["checksum_all"], (ranks, batch)


def test_column_shard_groups_times_frame_parallel_groups(cuda):
    """BASELINE configs[4] shape: S GPUs per frame x several frames in flight.  2 shards x 2 groups (and 2 x 1, 4 x 1) against the unsharded run,
    with and without CPW recalibration; a shard reads only the views that reach its window."""
    one = run("--gpus", 1, "--frames", 16, "--batch", 2)
    for ranks, shards in ((2, 2), (4, 2), (4, 4)):
        many = run(*multi(ranks), "--col-shards", shards, "--frames", 16, "--batch", 2)
        assert many["groups"] == ranks // shards and many["checksum_all"] == one["checksum_all"], (ranks, shards)
        assert min(many["views_read_per_rank"]) < one["views"]
    one = run("--gpus", 1, "--frames", 16, "--batch", 2, "--recalib-every", 8)
    many = run(*multi(4), "--col-shards", 2, "--frames", 16, "--batch", 2, "--recalib-every", 8)
    assert many["recalibrations_applied"] == 1 and many["checksum_all"] == one["checksum_all"]


def test_full_size_two_ranks(cuda):
    """config 2 at full size through two ranks (frame-parallel) and through a 2-shard group"""
    one = run("--gpus", 1, "--frames", 8, "--batch", 2, rig="cfg2")
    assert run(*multi(2), "--frames", 8, "--batch", 2, rig="cfg2")["checksum_all"] == one["checksum_all"]
    assert run(*multi(2), "--col-shards", 2, "--frames", 8, "--batch", 2, rig="cfg2")["checksum_all"] == one["checksum_all"]


def test_full_size_config5_two_shards_times_two_groups(cuda):
    """BASELINE configs[4] at FULL size (12 x 4K -> 7680 x 3840, 5 bands) in its own shape: 2 column shards per frame x 2 frame-parallel groups = 4 ranks
    (sharing the GPU over the host transport on a one-GPU box), against the single-rank run; plus the per-rank time breakdown the line carries."""
    one = run("--gpus", 1, "--frames", 4, "--batch", 1, rig="cfg5", timeout=1200)
    many = run(*multi(4), "--col-shards", 2, "--frames", 4, "--batch", 1, rig="cfg5", timeout=1200)
    assert many["groups"] == 2 and many["col_shards"] == 2 and many["frames"] == 4
    assert many["checksum_all"] == one["checksum_all"]
    assert max(many["views_read_per_rank"]) < one["views"]                 # a shard uploads only the views that reach its window (7 and 8 of 12)
    assert len(many["per_rank"]) == 4 and all(t["stitch_gpu_ms"] > 0 and t["wall_ms"] > 0 for t in many["per_rank"])
    assert many["per_rank"][2]["gather_stream_ms"] > 0                      # the second group's leader sent its slabs to the sink


def test_full_size_config3_recalibration_every_60_frames(cuda):
    """BASELINE configs[2] at full size through the multi-rank pipeline: CPW with 40 x 40 meshes, new meshes every 60 frames from rank 0's recalibration
    thread, broadcast one batch ahead -- 2 ranks x batches of 6 frames (swap at frame 60 = a batch boundary of both the 1- and the 2-rank run)."""
    args = ("--frames", 72, "--batch", 6, "--recalib-every", 60, "--mesh", "40x40")
    one = run("--gpus", 1, *args, rig="cfg2", timeout=1200)
    assert one["recalibrations_applied"] == 1 and one["cpw"] is True
    many = run(*multi(2), *args, rig="cfg2", timeout=1200)
    assert many["recalibrations_applied"] == 1 and many["checksum_all"] == one["checksum_all"]
    assert all(t["mesh_exchange_host_ms"] >= 0 for t in many["per_rank"]) and len(many["per_rank"]) == 2


def test_device_buffers_through_the_binding(ms, cuda):
    """msdist.Dist with device tensors: a one-rank communicator on RCCL (self send / recv in a group, broadcast, barrier) and, from two threads
    sharing the GPU, the host transport moving device memory."""
    import threading
    import msdist
    d = msdist.Dist(0, 1, msdist.unique_id(1, msdist.RCCL), device=0)
    info = d.info()
    assert info["transport"] == "rccl" and info["comm_nranks"] == 1
    a = torch.arange(1 << 20, dtype=torch.int32, device=cuda)
    b = torch.zeros_like(a)
    d.group_begin(); d.send(a, 0); d.recv(b, 0); d.group_end()
    d.broadcast(a, 0); d.barrier()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    d.close()
    idb = msdist.unique_id(2, msdist.HOST)
    res, errs = {}, []

    def rank(r):
        try:
            dd = msdist.Dist(r, 2, idb, device=0)
            mine = torch.full((3 * (1 << 20) + 7,), 40 + r, dtype=torch.uint8, device=cuda)
            got = torch.zeros_like(mine)
            dd.group_begin(); dd.send(mine, 1 - r); dd.recv(got, 1 - r); dd.group_end()
            slab = torch.full((1000,), 7 + r, dtype=torch.uint8, device=cuda)
            recv = [None, torch.zeros(1000, dtype=torch.uint8, device=cuda)] if r == 0 else None
            dd.gather_slabs(slab, recv, sink=0)
            torch.cuda.synchronize()
            res[r] = (int(got[0]), int(got[-1]), None if r else int(recv[1][0]))
            dd.barrier(); dd.close()
        except Exception as e:      # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join(timeout=180) for t in ts]
    assert not errs, errs
    assert res == {0: (41, 41, 8), 1: (40, 40, None)}


def test_rccl_communicator_beside_torchs_nccl_process_group(cuda):
    """bench.py --gpus N keeps torch.distributed (backend "nccl" = RCCL) for the barrier / max-over-ranks of the bench contract and moves the slabs through ms_dist's own
    RCCL communicator: both live in one process.  One rank is all a one-GPU box offers -- the two communicators are created, used and destroyed side by side in a
    child process (torch's process group cannot be re-created inside pytest's)."""
    code = r'''
import os, sys, torch
sys.path.insert(0, os.path.join(%r, "video-stitcher_amd"))
import torch.distributed as dist
import msdist
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
t = torch.ones(8, device="cuda"); dist.all_reduce(t); dist.barrier()
box = [msdist.unique_id(1, msdist.RCCL)]
dist.broadcast_object_list(box, src=0)
d = msdist.Dist(0, 1, box[0], device=0)
info = d.info()
a = torch.arange(1 << 18, dtype=torch.int32, device="cuda"); b = torch.zeros_like(a)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    d.group_begin(); d.send(a, 0); d.recv(b, 0); d.group_end()
side.synchronize()
dist.all_reduce(t); dist.barrier(); torch.cuda.synchronize()
assert torch.equal(a, b) and float(t[0]) == 1.0 and info["transport"] == "rccl" and info["comm_nranks"] == 1
# ONE RCCL per process (VERDICT r05 item 5b): the file the product resolved its entry points from is the very librccl torch's initialised NCCL process group runs on
# (PyTorch ships its own copy under the same soname; a second copy beside it would mean two sets of RCCL globals / proxy threads in one process)
mapped = sorted({l.split()[-1] for l in open("/proc/self/maps") if "librccl" in l})
assert len(mapped) == 1 and os.path.realpath(mapped[0]) == info["librccl_path"] == msdist.rccl_library_path(), (mapped, info["librccl_path"])
d.close(); dist.destroy_process_group()
print("OK", info["rccl_version"])
''' % ROOT
    out = subprocess.run([os.sys.executable, "-c", code], capture_output=True, timeout=300)
    assert out.returncode == 0 and b"OK" in out.stdout, (out.stdout.decode()[-500:], out.stderr.decode()[-1500:])


# ---- the RCCL branch of csrc/dist.cpp with N > 1 ranks on a one-GPU box ---------------------------------------------------
# The real library refuses two ranks on one device, so ncclCommInitRank / Send / Recv / Broadcast / AllGather / GroupStart / End are served by the loopback
# implementation tests/fake_rccl.cpp (stream-ordered and asynchronous like NCCL, bytes through shared memory), handed to the product through
# ms_dist_set_rccl_library (`stitch_dist --rccl-lib`).  This proves call order, grouping, and the comm-stream / stitch-stream event ordering of the callers;
# RCCL over xGMI itself stays UNMEASURED until an N-GPU node runs it.
FAKE_RCCL = os.path.join(ROOT, "tests", "_fake_rccl", "libfake_rccl.so")


def fake(n):
    assert os.path.isfile(FAKE_RCCL), "tests/_fake_rccl/libfake_rccl.so is built by __graft_entry__.build()"
    return ["--gpus", n, "--share-gpu", "--transport", "rccl", "--rccl-lib", FAKE_RCCL]


# The loopback library waits for a transfer on the calling thread, not with a kernel on the stream: HIP multiplexes the streams of a process over a few
# hardware queues, and with every rank of stitch_dist in ONE process on ONE device a rank's waiting kernel would sit in front of the very kernels of
# another rank that it waits for -- a deadlock that separate GPUs cannot have.  So the runs need no queue settings of their own.  The received bytes still
# reach their buffer in the order of the caller's stream (a copy out of pinned staging, enqueued there): a consumer that skips the dependency reads stale
# bytes (test_rccl_consumer_that_skips_the_dependency_reads_stale_bytes).  Not covered: a send buffer reused before its stream has passed the send.
FAKE_ENV = dict(os.environ)


def _is_fake_rccl(res, ranks):
    d = res["dist"]
    return (d["transport"] == "rccl" and d["nranks"] == ranks and d["comm_nranks"] == ranks and d["rccl_version"] == 29999
            and os.path.realpath(d["librccl_path"]) == os.path.realpath(FAKE_RCCL))      # (stitch_dist prints the file the entry points were resolved from)


@pytest.mark.parametrize("ranks,batch", [(2, 4), (4, 2), (4, 1)])
def test_rccl_branch_frame_parallel_over_the_loopback_library(cuda, ranks, batch):
    one = run("--gpus", 1, "--frames", 16, "--batch", 4)
    many = run(*fake(ranks), "--frames", 16, "--batch", batch, env=FAKE_ENV)
    assert _is_fake_rccl(many, ranks) and many["frames"] == 16
    assert many["checksum_all"] == one["checksum_all"]


def test_rccl_branch_column_shards_recalibration_and_table_blob_over_the_loopback_library(cuda):
    one = run("--gpus", 1, "--frames", 16, "--batch", 4)
    # 2 column shards x 2 frame-parallel groups: ungrouped ncclSend of the windows to the leader on the stitch stream, grouped ncclRecv there, leaders -> sink on the comm stream
    res = run(*fake(4), "--col-shards", 2, "--frames", 16, "--batch", 2, env=FAKE_ENV)
    assert _is_fake_rccl(res, 4) and res["checksum_all"] == one["checksum_all"]
    # the mesh broadcast (host payload staged through device memory: ncclBroadcast) with the agreed swap frame, inside and outside column-shard groups
    cp = run("--gpus", 1, "--frames", 32, "--batch", 4, "--recalib-every", 8, "--mesh", "9x11")
    for extra in ([], ["--col-shards", 2]):
        res = run(*fake(4), *extra, "--frames", 32, "--batch", 4 if extra else 2, "--recalib-every", 8, "--mesh", "9x11", env=FAKE_ENV)
        assert _is_fake_rccl(res, 4) and res["recalibrations_applied"] == cp["recalibrations_applied"] == 3 and res["checksum_all"] == cp["checksum_all"], extra
    # the table blob from rank 0 (rank 0 calibrates -- hipDeviceSynchronize inside -- while the other rank threads wait for the blob in ncclBroadcast: on the host, so
    # nothing of theirs holds the device)
    res = run(*fake(2), "--frames", 16, "--batch", 4, "--tables-from-rank0", env=FAKE_ENV)
    assert _is_fake_rccl(res, 2) and res["checksum_all"] == one["checksum_all"]


def _exchange_rccl(rank, world, idb, fake_lib, q):
    """what every rank PROCESS runs over the loopback library: device buffers, ms_dist's RCCL branch"""
    try:
        import msdist
        import msstitch as ms
        msdist.set_rccl_library(fake_lib)
        torch.cuda.set_device(0)
        dev = torch.device("cuda:0")
        d = msdist.Dist(rank, world, idb, device=0)
        try:
            info = d.info()
            assert info["transport"] == "rccl" and info["nranks"] == world and info["comm_nranks"] == world and info["rccl_version"] == 29999 and info["devices"] == [0] * world
            with pytest.raises(ms.MsError):
                msdist.set_rccl_library(None)                 # too late: RCCL is resolved
            nxt, prv = (rank + 1) % world, (rank - 1) % world
            for k, n in enumerate((0, 1, 4097, (1 << 20) + 13, 3 * (1 << 20) + 5)):      # ring, incl. an empty message and several mailbox pieces
                out = torch.full((n,), (17 * rank + k) % 251, dtype=torch.uint8, device=dev)
                got = torch.zeros(n, dtype=torch.uint8, device=dev)
                d.group_begin(); d.send(out, nxt); d.recv(got, prv); d.group_end()
                torch.cuda.synchronize()
                assert bool(torch.all(got == (17 * prv + k) % 251)), (rank, k)
            # two sends and two receives per peer, and a send to oneself, in ONE group; the buffers are filled by kernels enqueued just before (stream order, no host sync)
            n2 = 5 * (1 << 19)
            a_out = [torch.empty(n2, dtype=torch.uint8, device=dev).fill_((3 + 2 * rank + 7 * r) % 251) for r in range(world)]
            b_out = [torch.empty(n2 + 1, dtype=torch.uint8, device=dev).fill_((4 + 2 * rank + 7 * r) % 251) for r in range(world)]
            a_in = [torch.zeros(n2, dtype=torch.uint8, device=dev) for _ in range(world)]
            b_in = [torch.zeros(n2 + 1, dtype=torch.uint8, device=dev) for _ in range(world)]
            d.group_begin()
            for r in range(world):
                d.recv(a_in[r], r); d.send(a_out[r], r); d.send(b_out[r], r); d.recv(b_in[r], r)
            d.group_end()
            sums = [(a_in[r].sum(dtype=torch.int64), b_in[r].sum(dtype=torch.int64)) for r in range(world)]      # consumers enqueued right behind the group
            torch.cuda.synchronize()
            for r in range(world):
                assert int(sums[r][0]) == n2 * ((3 + 2 * r + 7 * rank) % 251) and int(sums[r][1]) == (n2 + 1) * ((4 + 2 * r + 7 * rank) % 251), (rank, r)
            # broadcasts: device buffer in place; a 5 MB HOST payload (staged through device memory, the staging buffer grows: the table blob's path)
            t = torch.arange(100000, dtype=torch.float32, device=dev) * (1.0 if rank == world - 1 else 0.0)
            d.broadcast(t, world - 1)
            torch.cuda.synchronize()
            assert bool(torch.equal(t, torch.arange(100000, dtype=torch.float32, device=dev)))
            h = (np.arange(5 * (1 << 20), dtype=np.uint32) * 2654435761 % 251).astype(np.uint8) if rank == 0 else np.zeros(5 * (1 << 20), np.uint8)
            d.broadcast(h, 0)
            assert np.array_equal(h, (np.arange(5 * (1 << 20), dtype=np.uint32) * 2654435761 % 251).astype(np.uint8))
            d.barrier()
            # the frame gather on a side stream with event ordering, as bench.py drives it
            slab = torch.full((3, 1 << 20), 40 + rank, dtype=torch.uint8, device=dev)
            recv = [torch.zeros_like(slab) for _ in range(world)] if rank == 0 else None
            cs = torch.cuda.Stream(device=dev)
            cs.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cs):
                d.gather_slabs(slab, recv, sink=0)
            cs.synchronize()
            if rank == 0:
                for r in range(1, world):
                    assert bool(torch.all(recv[r] == 40 + r)), r
            n_views, rows, cols = 3, 5, 7
            assert d.mesh_exchange(0, None, n_views, rows, cols) is None
            rng = np.random.default_rng(5)
            mx, my = rng.random((n_views, rows, cols), dtype=np.float32), rng.random((n_views, rows, cols), dtype=np.float32)
            got = d.mesh_exchange(0, (4800, 2, mx, my) if rank == 0 else None, n_views, rows, cols)
            assert got is not None and got[0] == 4800 and got[1] == 2 and np.array_equal(got[2], mx) and np.array_equal(got[3], my)
            d.barrier()
        finally:
            d.close()
        q.put((rank, "ok"))
    except Exception as e:      # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()[-1500:] or repr(e)))


@pytest.mark.parametrize("world", [2, 3])
def test_rccl_branch_between_processes_over_the_loopback_library(cuda, world):
    """ms_dist's RCCL branch call by call, one PROCESS per rank (all on device 0): grouped and ungrouped ncclSend / ncclRecv with stream-ordered producers and
    consumers, a send to oneself, ncclBroadcast in place and staged from host memory (5 MB), the barrier's all-gather, the frame gather on a side stream, the mesh exchange."""
    import msdist
    import torch.multiprocessing as mp
    assert os.path.isfile(FAKE_RCCL)
    ctx = mp.get_context("spawn")
    q0 = ctx.Queue()

    # (the id comes from a process that has the loopback library set: this process keeps the real RCCL for the other tests)
    idp = ctx.Process(target=_make_fake_id, args=(world, FAKE_RCCL, q0))
    idp.start()
    idb = q0.get(timeout=120)
    idp.join(timeout=60)
    assert isinstance(idb, bytes) and msdist.id_transport(idb) == msdist.RCCL, idb
    q = ctx.Queue()
    procs = [ctx.Process(target=_exchange_rccl, args=(r, world, idb, FAKE_RCCL, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert got == {r: "ok" for r in range(world)}, got


def _stale_consumer_rccl(rank, idb, fake_lib, go, q):
    """rank 1 receives 64 MiB from rank 0 on stream `cs`.  While its thread waits in ncclRecv (the proxy is done only once rank 0 sends), a second thread enqueues
    about a second of matmuls on `cs` and only then lets rank 0 send: the copy into the destination lands on `cs` behind that work.  A consumer on another stream
    that skips the dependency runs at once and must see the old bytes; the one that waits for `cs` must see the new ones."""
    try:
        import threading
        import msdist
        msdist.set_rccl_library(fake_lib)
        torch.cuda.set_device(0)
        dev = torch.device("cuda:0")
        n = 64 << 20
        d = msdist.Dist(rank, 2, idb, device=0)
        try:
            if rank == 0:
                out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                assert go.wait(120)
                d.send(out, 1)
                torch.cuda.synchronize()
                q.put((rank, "ok"))
                return
            got = torch.zeros(n, dtype=torch.uint8, device=dev)
            x = torch.randn(8192, 8192, device=dev)
            cs = torch.cuda.Stream(device=dev)
            side = torch.cuda.Stream(device=dev, priority=-1)      # (another priority level: never behind `cs` in a shared hardware queue)
            torch.cuda.synchronize()

            def hold_cs():
                time.sleep(1.0)                                    # the main thread is inside ncclRecv by now: its ready event precedes what follows
                with torch.cuda.stream(cs):
                    for _ in range(100):
                        torch.mm(x, x)
                go.set()
            t = threading.Thread(target=hold_cs)
            t.start()
            with torch.cuda.stream(cs):
                d.recv(got, 0)
            t.join()
            with torch.cuda.stream(side):                          # the defect: no wait for `cs`
                early = int(got.sum(dtype=torch.int64))
            busy = not cs.query()
            side.wait_stream(cs)
            with torch.cuda.stream(side):                          # the correct consumer
                late = int(got.sum(dtype=torch.int64))
            q.put((rank, "ok" if (early == 0 and late == 7 * n) else "early %d late %d (of %d) cs busy after the early read: %s" % (early, late, 7 * n, busy)))
        finally:
            d.close()
    except Exception as e:      # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()[-1500:] or repr(e)))


def test_rccl_consumer_that_skips_the_dependency_reads_stale_bytes(cuda):
    """The loopback library keeps the post-transfer side of NCCL's stream semantics: what ncclRecv delivers reaches the destination in the order of the caller's
    stream, so a consumer on another stream that does not wait for it reads the bytes that were there before -- the defect the checksum tests of this file would
    then catch -- and one that waits reads the received bytes."""
    import msdist
    import torch.multiprocessing as mp
    assert os.path.isfile(FAKE_RCCL)
    ctx = mp.get_context("spawn")
    q0 = ctx.Queue()
    idp = ctx.Process(target=_make_fake_id, args=(2, FAKE_RCCL, q0))
    idp.start()
    idb = q0.get(timeout=120)
    idp.join(timeout=60)
    assert isinstance(idb, bytes) and msdist.id_transport(idb) == msdist.RCCL, idb
    q, go = ctx.Queue(), ctx.Event()
    procs = [ctx.Process(target=_stale_consumer_rccl, args=(r, idb, FAKE_RCCL, go, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert got == {0: "ok", 1: "ok"}, got


def _make_fake_id(world, fake_lib, q):
    try:
        import msdist
        msdist.set_rccl_library(fake_lib)
        q.put(msdist.unique_id(world, msdist.RCCL))
    except Exception as e:      # noqa: BLE001
        q.put(repr(e))


def test_rccl_branch_full_size_config2_over_the_loopback_library(cuda):
    """BASELINE configs[3]'s shape at full size: 6 x 1080p -> 3840 x 1920, 4 frame-parallel ranks, 3.6 MB I420 slabs per frame through ncclSend / ncclRecv."""
    one = run("--gpus", 1, "--frames", 8, "--batch", 2, rig="cfg2")
    res = run(*fake(4), "--frames", 8, "--batch", 1, rig="cfg2", env=FAKE_ENV)
    assert _is_fake_rccl(res, 4) and res["checksum_all"] == one["checksum_all"]
