#!/usr/bin/env python3
"""Headline benchmark: frames/sec at 600x1000, 32 ROI/frame (BASELINE.json).

A "step" is one pass of the hot path over one batch of synthetic frames already resident in HBM.

  --config sgg              (default, the headline) BASELINE.json configs[1]: cfgs/res101.yml, 2 frames/GPU, 32 boxes +
                            32 relation pairs per frame, SGG_emb forward + backward + SGD (trainval_net_SGG_emb.py:189-255).
                            With --gpus 8 this is configs[3] (16 frames over 8 GPUs, RCCL exchange of the vrd gradients).
  --config instance_styled  configs[2]: instance_styleD D+G adversarial step, 4 source + 4 target frames/GPU, all of
                            layer1-3 + heads trained (trainval_net_instance_styleD_bilinear.py:262-341).
  --config joint            configs[4]: one instance_styleD step followed by one SGG_emb step on 4 frames/GPU.
  --config res50            configs[0]: cfgs/res50.yml, ONE 600x1000 frame, Faster-RCNN forward + SGG_emb head forward
                            (the reference's CPU-runnable plumbing case, here on the GPU and checked against the oracle).

Prints ONE JSON line on rank 0 (the contract of the task brief).  A plain run measures the headline only: set-up, --warmup
steps, --steps timed steps, the line (``value``, ``ms_per_step`` = milliseconds per timed step).  --full adds everything
else: the roofline blocks (eager steps profiled with HIP events), and for the single-GPU sgg config the "also" measurements
(the loader-fed step, the ROI / NMS ops and roofline_hbm, configs[2], the test loops) and the CPU baseline.

--dump-outputs DIR writes what the timed path computed in its last step as DIR/<name>.npy (float32, float64 for integer
data; a fixed, seeded sample of the larger arrays, 64 MB at most): the loss(es), the trained parameters after the step's
update and, for the relation step, the backbone's feature maps.  The inputs are seeded: two builds compare output for output.

--gpus N without a torchrun environment starts its own N ranks (one process per GPU, RCCL over xGMI, rendezvous on
127.0.0.1) and exits non-zero if any rank fails to come up; under torchrun (RANK set) it is one of the ranks.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# before the HIP runtime initialises (i2vsgg_amd/__init__.py explains)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

MFMA_F32_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
HBM_PEAK_GBS = 8000.0             # same guide, "HBM3E peak BW" (spec)
SET_CFGS = ["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30",
            "TRAIN.BATCH_SIZE", "32", "TRAIN.RPN_POST_NMS_TOP_N_TARGET", "32"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="sgg", choices=["sgg", "instance_styled", "joint", "res50"])
    ap.add_argument("--data", default="resident", choices=["resident", "loader", "loader_u8"],
                    help="resident: one synthetic minibatch resident in HBM (the headline); loader: roibatchLoader minibatches of "
                         "varying size staged from pinned host memory every step (config sgg; with --full also reported beside the "
                         "headline)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a HIP graph")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline blocks, the 'also' legs, the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-also", action="store_true", help="with --full: skip the 'also' measurements")
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--dump-launches", default="", help="with --full: write one line per GEMM launch of a profiled step")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path computed in its last step as DIR/<name>.npy")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous rehearsal on the CPU (gloo): no GPU work, prints the line with dry_run")
    return ap.parse_args()


# ----------------------------------------------------------------------------- launcher
def launch_ranks(n):
    """Start n copies of this script, one per GPU, and wait.  Runs BEFORE anything in this process touches the GPU."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), I2V_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            r = p.poll()
            if r is None:
                continue
            alive.remove(p)
            if r != 0 and rc == 0:
                rc = r if r > 0 else 1
                for q in alive:             # one rank down: the others would wait in a collective for ever
                    q.terminate()
        time.sleep(0.05)
    if rc:
        sys.stderr.write("bench.py: a rank exited with %d (%d ranks requested)\n" % (rc, n))
    sys.exit(rc)


# ----------------------------------------------------------------------------- CPU baseline
def cpu_baseline(threads_list):
    """The CPU oracle (a port: oracle/nets.py, torch-CPU fp32) on a bounded sample of the configs[1] workload: ONE
    600x1000 frame through the ResNet-101 C4 backbone + the relation head forward, backward and SGD update for that
    frame's 32 boxes + 32 pairs.  BASELINE.md section 3 protocol: 2 warm-up + 5 timed iterations, median, at every thread
    count of ``threads_list``."""
    import numpy as np
    import torch
    from i2vsgg_amd import synthetic as syn, train
    from i2vsgg_amd.model.faster_rcnn.faster_rcnn_SGG_emb import build_pair_tables
    from oracle import nets
    p = syn.backbone_params(0, 101, top=False)
    v = {k: t.requires_grad_() for k, t in syn.vrd_params(13).items()}
    im, info, annos = train.synthetic_sgg_batch(1, 1)
    gt, union, bounds, labels, ixs, ixo = build_pair_tables(annos["f0"], 1.0, 600.0, 1000.0, 62)
    boxes = np.zeros((gt.shape[0], 5), np.float32); boxes[:, 1:] = gt
    relb = np.zeros((union.shape[0], 5), np.float32); relb[:, 1:] = union
    masks = np.zeros((union.shape[0], 2, 32, 32), np.float32)
    for i in range(union.shape[0]):
        for j in range(2):
            x1, y1, x2, y2 = bounds[i, j]
            masks[i, j, y1:y2, x1:x2] = 1
    prd = syn.word_vectors(21, 62)
    opt = torch.optim.SGD(list(v.values()), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    out = {}
    for threads in threads_list:
        torch.set_num_threads(threads)
        times = []
        for it in range(7):
            t0 = time.perf_counter()
            with torch.no_grad():
                fmap, _ = nets.extract_feature(torch.from_numpy(im), p)
            sc, _ = nets.vrd_head(fmap, boxes, relb, masks, ixs, ixo, prd, v, training=True)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(sc, torch.from_numpy(labels))
            opt.zero_grad()
            loss.backward()
            opt.step()
            if it >= 2:
                times.append(time.perf_counter() - t0)
        out[threads] = sorted(times)[len(times) // 2]
    return out


def _median_time(fn, warm=2, timed=5):
    ts = []
    for it in range(warm + timed):
        t0 = time.perf_counter()
        fn()
        if it >= warm:
            ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def cpu_baseline_stages(threads):
    """the CPU oracle stage by stage at ``threads`` torch threads, ONE 600x1000 frame / 32 ROIs (2
    warm-up + 5 timed, median; the two stages that take seconds per pass -- the vrd head 1 + 3, the configs[2] D+G step 1 + 2 --
    so that the whole CPU leg stays near 30 s): backbone fwd, RPN head + proposal layer (decode, sort, the
    reference's greedy NMS 12000 -> 2000), RoIAlignAvg fwd / bwd, layer4 head, netD_pixel and netD_style fwd + bwd, vrd head
    fwd + bwd, and the instance_styleD D+G step on 1 source + 1 target frame (every stage under autograd, SGD update).
    -> {stage: {"ms": median, "frames_per_s": ...}}.  ROIAlign / ROIPool / NMS are the oracle's C (one thread)."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from i2vsgg_amd import synthetic as syn, train
    from i2vsgg_amd.model.faster_rcnn.faster_rcnn_SGG_emb import build_pair_tables
    from oracle import cops, nets, rpn
    torch.set_num_threads(threads)
    p = {}
    p.update(syn.backbone_params(0, 101, top=True))
    p.update(syn.rpn_params(10, std=0.02))
    p.update(syn.det_head_params(11, 16))
    p.update(syn.netd_params(12))
    im, info = syn.frames(3, 1, 600, 1000)
    imt, _ = syn.frames(103, 1, 600, 1000)
    gt, nb = syn.gt_boxes(3, 1, 8, 16, 30, 600, 1000)
    x = torch.from_numpy(im)
    out = {}
    with torch.no_grad():
        feat, feat1 = nets.extract_feature(x, p)
        out["backbone_fwd"] = _median_time(lambda: nets.extract_feature(x, p))

        def rpn_stage():
            cls, prob, box = nets.rpn_head(feat, p)
            return rpn.proposal_layer(prob[:, 9:].numpy(), box.numpy(), info, 12000, 2000, 0.7)
        rois_all, _ = rpn_stage()
        out["rpn_head_proposal_nms"] = _median_time(rpn_stage)
    rois = np.ascontiguousarray(rois_all[0, :32]).astype(np.float32)
    fnp = feat.numpy()
    pooled_np = cops.roi_align_avg_fwd(fnp, rois, 7, 7, 1.0 / 16.0)
    out["roi_align_avg_fwd"] = _median_time(lambda: cops.roi_align_avg_fwd(fnp, rois, 7, 7, 1.0 / 16.0))
    try:        # the one stage whose REFERENCE code exists as a binary: ROIAlignForwardCpu (roi_align.c:80-136) from oracle/_ref,
                # where that built artefact travelled, + avg_pool2d as RoIAlignAvg does (kind "reference" for this stage alone)
        from oracle import build_ref
        if build_ref.available():
            out["roi_align_avg_fwd_reference_c"] = _median_time(lambda: torch.nn.functional.avg_pool2d(
                torch.from_numpy(build_ref.roi_align_fwd(fnp, rois, 8, 8, 1.0 / 16.0)), kernel_size=2, stride=1))
    except Exception:            # noqa: BLE001 -- an optional extra
        pass
    g = np.ones_like(pooled_np)
    out["roi_align_avg_bwd"] = _median_time(lambda: cops.roi_align_avg_bwd(g, rois, fnp.shape, 1.0 / 16.0))
    pooled = torch.from_numpy(pooled_np)
    with torch.no_grad():
        out["layer4_head_fwd"] = _median_time(lambda: nets.head_to_tail(pooled, p))
    train_keys = [k for k in p if (k.startswith("netD_") or k.startswith("RCNN_rpn") or k.startswith("RCNN_cls") or
                                   k.startswith("RCNN_bbox") or ((".conv" in k or "downsample.0" in k) and not k.startswith("RCNN_base.0")))]
    for k in train_keys:
        p[k].requires_grad_()

    def zero():
        for k in train_keys:
            p[k].grad = None

    def dpix():
        zero()
        (0.5 * (nets.netd_pixel(pooled, p, 0.1) ** 2).mean()).backward()
    out["netD_pixel_fwd_bwd"] = _median_time(dpix)
    f1 = feat1.detach()

    def dsty():
        zero()
        (0.5 * (nets.netd_style(f1, p, 0.001) ** 2).mean()).backward()
    out["netD_style_fwd_bwd"] = _median_time(dsty)
    # vrd head, 32 boxes + 32 pairs (the relation step's head; its end-to-end figure is cpu_baseline.value)
    v = {k: t.requires_grad_() for k, t in syn.vrd_params(13).items()}
    _, _, annos = train.synthetic_sgg_batch(1, 1)
    bx, union, bounds, labels, ixs, ixo = build_pair_tables(annos["f0"], 1.0, 600.0, 1000.0, 62)
    b5 = np.zeros((bx.shape[0], 5), np.float32); b5[:, 1:] = bx
    r5 = np.zeros((union.shape[0], 5), np.float32); r5[:, 1:] = union
    masks = train._rasterize_host(bounds, 2)
    prd = syn.word_vectors(21, 62)

    def vrd():
        for t in v.values():
            t.grad = None
        sc, _ = nets.vrd_head(fnp, b5, r5, masks, ixs, ixo, prd, v, training=True)
        F.binary_cross_entropy_with_logits(sc, torch.from_numpy(labels)).backward()
    out["vrd_head_fwd_bwd"] = _median_time(vrd, warm=1, timed=3)

    # ---- configs[2] on the CPU: D+G step, 1 source + 1 target frame, every trained stage under autograd
    class RoiAlignAvg(torch.autograd.Function):
        @staticmethod
        def forward(ctx, f, r):
            ctx.r, ctx.shape = r, tuple(f.shape)
            return torch.from_numpy(cops.roi_align_avg_fwd(f.detach().numpy(), r, 7, 7, 1.0 / 16.0))

        @staticmethod
        def backward(ctx, go):
            return torch.from_numpy(cops.roi_align_avg_bwd(np.ascontiguousarray(go.numpy()), ctx.r, ctx.shape, 1.0 / 16.0)), None
    opt = torch.optim.SGD([p[k] for k in train_keys], lr=5e-4, momentum=0.9, weight_decay=5e-4)
    rs = np.random.RandomState(3)

    def side(frames, target):
        ft, ft1 = nets.extract_feature(frames, p)
        d_style = nets.netd_style(ft1, p, 0.001)
        cls, prob, box = nets.rpn_head(ft, p)
        post = 32 if target else 2000
        r_all, _ = rpn.proposal_layer(prob[:, 9:].detach().numpy(), box.detach().numpy(), info, 12000, post, 0.7)
        loss = 0.0
        if not target:
            fh, fw = ft.shape[2], ft.shape[3]
            L, T, IW, OW = rpn.anchor_target_layer(fh, fw, gt, info, rs)
            pair = cls.view(1, 2, 9 * fh, fw).permute(0, 2, 3, 1).reshape(-1, 2)
            lab = torch.from_numpy(L).reshape(-1)
            keep = lab.ne(-1).nonzero().view(-1)
            loss = F.cross_entropy(pair[keep], lab[keep].long())
            d = torch.from_numpy(IW) * (box - torch.from_numpy(T))
            ad = d.abs()
            near = (ad < 1.0 / 9.0).float()
            loss = loss + (torch.from_numpy(OW) * (d * d * 4.5 * near + (ad - 0.5 / 9.0) * (1 - near))).sum((1, 2, 3)).mean()
            rb, lab_o, tg, inw, outw = rpn.proposal_target_layer(r_all, gt, rs, batch_size=32)
            r32 = np.ascontiguousarray(rb.reshape(-1, 5)).astype(np.float32)
        else:
            r32 = np.ascontiguousarray(r_all.reshape(-1, 5)).astype(np.float32)
        pl = RoiAlignAvg.apply(ft, r32)
        d_inst = nets.netd_pixel(pl, p, 0.1)
        if target:
            return 0.5 * ((1 - d_inst) ** 2).mean() + 0.5 * ((1 - d_style) ** 2).mean()
        h = nets.head_to_tail(pl, p)
        lo = torch.from_numpy(lab_o.reshape(-1)).long()
        bp = F.linear(h, p["RCNN_bbox_pred.weight"], p["RCNN_bbox_pred.bias"])
        bp = torch.gather(bp.view(-1, 16, 4), 1, lo.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
        cs = F.linear(h, p["RCNN_cls_score.weight"], p["RCNN_cls_score.bias"])
        d = torch.from_numpy(inw.reshape(-1, 4)) * (bp - torch.from_numpy(tg.reshape(-1, 4)))
        ad = d.abs()
        near = (ad < 1.0).float()
        l_box = (torch.from_numpy(outw.reshape(-1, 4)) * (d * d * 0.5 * near + (ad - 0.5) * (1 - near))).sum(1).mean()
        return loss + F.cross_entropy(cs, lo) + l_box + 0.5 * (d_inst ** 2).mean() + 0.5 * (d_style ** 2).mean()

    def dg_step():
        opt.zero_grad()
        (side(x, False) + side(torch.from_numpy(imt), True)).backward()
        opt.step()
    out["instance_styled_dg_step_1+1_frames"] = _median_time(dg_step, warm=1, timed=2)
    res = {k: {"ms": 1e3 * t, "frames_per_s": (2.0 if k.startswith("instance_styled") else 1.0) / t} for k, t in out.items()}
    return res


def train_mod():
    from i2vsgg_amd import train
    return train


# ----------------------------------------------------------------------------- --dump-outputs
DUMP_MAX_BYTES = 64 << 20
_OUTPUTS = {}


def _host(t, cap, name):
    """One output on the host: float32 (float64 for float64 and integer data), as a fixed sample of ``cap`` elements of its
    flattened form when larger (seeded by the name: the same positions in every run)."""
    import numpy as np
    import torch
    t = t.detach()
    if cap is not None and t.numel() > cap:
        idx = np.unique(np.random.default_rng(zlib.crc32(name.encode())).integers(0, t.numel(), cap))
        t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
    t = t.cpu()
    return t.double().numpy() if (t.dtype == torch.float64 or not t.is_floating_point()) else t.float().numpy()


def keep_outputs(a, rank, fn):
    """--dump-outputs: ``fn() -> {name: tensor or (tensor, cap)}``, what the timed path computed in its last step, copied to
    the host right behind the timed region (before a --full measurement runs more steps on the same objects)."""
    if not a.dump_outputs or rank != 0:
        return
    import torch
    torch.cuda.synchronize()
    for name, v in fn().items():
        t, cap = v if isinstance(v, tuple) else (v, None)
        _OUTPUTS[name] = _host(t, cap, name)


def param_outputs(named, cap=None, budget=None):
    """The trained parameters (after the last step's update); ``budget`` elements spread evenly over them when given."""
    named = [(n, p) for n, p in named if p.requires_grad]
    if budget is not None:
        cap = max(1024, budget // max(len(named), 1))
    return {n: (p, cap) for n, p in named}


def write_outputs(d):
    import numpy as np
    total = sum(v.nbytes for v in _OUTPUTS.values())
    if total > DUMP_MAX_BYTES:
        raise RuntimeError("--dump-outputs: %d bytes over the %d-byte limit" % (total, DUMP_MAX_BYTES))
    os.makedirs(d, exist_ok=True)
    for name, v in sorted(_OUTPUTS.items()):
        np.save(os.path.join(d, name + ".npy"), v)


# ----------------------------------------------------------------------------- measurement helpers
def timed_steps(step_fn, warmup, steps, dev):
    import torch
    from i2vsgg_amd import parallel
    for _ in range(warmup):
        step_fn()
    parallel.barrier(dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step_fn()
    torch.cuda.synchronize(dev)
    parallel.barrier(dev)
    return parallel.max_over_ranks(time.perf_counter() - t0, dev)


def profile_eager(body, n_prof, dev):
    """HIP events (on the launch stream) around every GEMM-shaped launch of ``n_prof`` eager steps of the same objects:
    events cannot be read back from inside a graph replay."""
    import torch
    from i2vsgg_amd import ops
    # An event pair brackets (idle time until the launch arrives) + (the kernel): with the device waiting for a host that
    # needs 15-25 us of Python per launch, the pairs of 30-us kernels read 32-38 us depending on the box's CPU.  A ~10 ms
    # GEMM in front of every profiled step keeps the device busy while the host queues the step behind it, so a pair
    # measures its kernel (rocprofv3's durations of the same launches are the cross-check, profiles/README.md).
    a = torch.randn(8192, 8192, device=dev)
    ops.PROFILE = []
    for _ in range(n_prof):
        torch.mm(a, a)
        body()
    torch.cuda.synchronize(dev)
    del a
    rec, ops.PROFILE = ops.PROFILE, None
    return [dict(t=e0.elapsed_time(e1) * 1e-3, flops=fl, tag=tag, desc=d, bytes=by) for e0, e1, fl, tag, d, by in rec]


def record_is_current(rec):
    """A committed rocprofv3 summary names the kernel sources it measured (``source_digests``, rounds 6+): it is quoted only
    while those files are the ones this library was built from.  Older records carry no digests and are quoted as they are
    (their file name says which round's kernels they saw)."""
    want = rec.get("source_digests")
    if not want:
        return True
    from i2vsgg_amd import build as _b
    try:
        return _b.source_digests(sorted(want)) == want
    except OSError:
        return False


def pmc_traffic(kernel_key, names=("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json", "r01_pmc_summary.json")):
    """HBM bytes per launch of the dominant kernel from the PMC passes committed under profiles/ (rocprofv3 cannot run inside
    the timed process): the newest record whose kernel sources are the loaded library's; None when there is none."""
    for name in names:
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            try:
                with open(path) as f:
                    rec = json.load(f)
                if not record_is_current(rec):
                    continue
                return rec[kernel_key]["hbm_bytes_per_launch_corrected"], "profiles/" + name
            except Exception:
                continue
    return None, None


def by_kind(rec, n_prof):
    agg = {}
    for r in rec:
        d = agg.setdefault(r["tag"], [0.0, 0.0, 0])
        d[0] += r["t"]; d[1] += r["flops"]; d[2] += 1
    return {k: {"ms_per_step": 1e3 * v[0] / n_prof, "tflops": v[1] / max(v[0], 1e-12) / 1e12, "launches": v[2] // n_prof}
            for k, v in agg.items()}


# ----------------------------------------------------------------------------- the metric's second half: ROI ops / NMS
ROI_NMS_CASES = ("roi_align_avg_fwd_1x32", "roi_align_avg_bwd_1x32", "roi_align_avg_fwd_4x32", "roi_align_avg_bwd_4x32",
                 "roi_pool_geom_fwd_2x64", "nms_12000_to_2000", "nms_6000_to_300")
ROI_NMS_PMC = ("r06_roi_nms_pmc.json", "r05_roi_nms_pmc.json")
COLD_BYTES = 512 << 20          # a rotation's working set: twice the 256 MiB Infinity Cache


def roi_nms_case(dev, name, cold=False):
    """ONE HBM-side op of the path at the headline sizes -> dict(fn, sets, nbytes, kernels).  ``fn(i)`` launches the op once on
    buffer set ``i % sets`` and returns what must stay alive.  Only this case's buffers are built and nothing of the op is
    launched here except -- for a backward case -- the one forward per set its autograd node needs (another kernel: it never
    enters the backward's rows).  Shared with tools/roi_nms_pmc_one.py, so that the PMC passes profile exactly these launches.

    Two cache states: warm (``cold=False``: one set, launched back to back -- maps and outputs come out of the 256 MiB Infinity
    Cache, which is how the op runs inside a step, right behind the layer that wrote its map) and cold (a rotation over enough
    distinct maps AND outputs to exceed twice the Infinity Cache: every byte comes from / goes to HBM).

    ``kernels``: kernel name -> launches per op (exactly).  Algorithmic bytes: SURVEY.md 8(d) -- feature maps read once + output
    written once (ROIAlign: 9.81 MB + R * 1024 * 49 * 4 B per frame, the backward the same bytes reversed; ROIPool additionally
    writes its argmax); NMS: the reference algorithm's bytes 20 N + 2 * 8 * N * ceil(N / 64) (boxes + the 64-bit suppression
    mask written, then read)."""
    import numpy as np
    import torch
    from i2vsgg_amd import ops, synthetic as syn
    R = 32

    def n_sets(per_set):
        return max(2, -(-COLD_BYTES // per_set)) if cold else 1

    if name.startswith("roi_align_avg_"):
        B = int(name.rsplit("_", 1)[1].split("x")[0])
        bwd = "_bwd_" in name
        nbytes = B * 1024 * 38 * 63 * 4 + B * R * 1024 * 49 * 4
        rois = np.zeros((B * R, 5), np.float32)
        for b in range(B):
            rois[b * R:(b + 1) * R, 0] = b
            rois[b * R:(b + 1) * R, 1:] = syn.boxes(b, R)
        rt = torch.from_numpy(rois).to(dev)
        sets = n_sets(nbytes)
        feats = [torch.randn(B, 1024, 38, 63, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(sets)]
        if not bwd:
            return dict(fn=lambda i: ops.roi_align(feats[i % sets], rt, 7, 7, 1 / 16.0, avg=True), sets=sets, nbytes=nbytes,
                        kernels={"roi_align_fwd_roi_kernel": 1})
        for f in feats:
            f.requires_grad_()
        outs = [ops.roi_align(f, rt, 7, 7, 1 / 16.0, avg=True) for f in feats]
        gouts = [torch.randn_like(o) for o in outs]

        def run(i):
            f = feats[i % sets]
            f.grad = None                                   # the gradient map is written, not accumulated: a fresh block per set
            outs[i % sets].backward(gouts[i % sets], retain_graph=True)
            return f.grad
        return dict(fn=run, sets=sets, nbytes=nbytes, kernels=dict(ops.ROIALIGN_BWD_KERNELS))
    if name == "roi_pool_geom_fwd_2x64":
        # ROIPool as the captured relation step runs it: 2 packed frames, 32 boxes + 32 union boxes each, NCHW out for vrd.fc6,
        # extent of the maps read on the device (i2v_roi_pool_fwd_geom)
        Bp, Rp, C, h, w = 2, 64, 1024, 38, 63
        nbytes = Bp * C * h * w * 4 + 2 * Bp * Rp * C * 49 * 4
        sets = n_sets(nbytes)
        ext = torch.tensor([h, w], dtype=torch.int32, device=dev)
        maps = [ops.PackedMaps(torch.randn(Bp * h * w * C, device=dev), Bp, C, ext) for _ in range(sets)]
        rp = np.zeros((Bp * Rp, 5), np.float32)
        for b in range(Bp):
            rp[b * Rp:(b + 1) * Rp, 0] = b
            rp[b * Rp:(b + 1) * Rp, 1:] = syn.boxes(10 + b, Rp)
        rpt = torch.from_numpy(rp).to(dev)
        return dict(fn=lambda i: ops.roi_pool_packed(maps[i % sets], rpt, 7, 7, 1 / 16.0, out_nchw=True), sets=sets, nbytes=nbytes,
                    kernels={"roi_pool_fwd_c128_kernel": 1})
    if name.startswith("nms_"):
        n, keep = int(name.split("_")[1]), int(name.split("_")[3])
        nbytes = 20 * n + 2 * 8 * n * ((n + 63) // 64)
        sets = n_sets(nbytes)
        base = syn.tie_free_dets(n, n, clustered=True)
        dets = [torch.from_numpy(base).to(dev) for _ in range(sets)]
        # cold: the op's 18 MB mask lives in a per-stream workspace, written and read back inside the op -- the rotation can
        # only renew the boxes; the mask round trip stays where the hardware keeps it (stated in the line)
        return dict(fn=lambda i: ops.nms_sorted(dets[i % sets], 0.7, keep), sets=sets, nbytes=nbytes, kernels=dict(ops.NMS_KERNELS))
    raise KeyError(name)


def time_roi_nms_case(dev, case, blocker, reps=20):
    """us per op: ONE HIP-event pair on the launch stream around back-to-back launches (whole rotations in the cold state),
    queued behind a ~10 ms blocker GEMM so that the pair brackets device time and not the host's launch latency."""
    import torch
    sets = case["sets"]
    reps = max(reps, sets) // sets * sets
    ring = [None] * sets
    for i in range(max(3, sets)):
        ring[i % sets] = case["fn"](i)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(blocker, blocker)
    e0.record()
    for i in range(reps):
        ring[i % sets] = case["fn"](i)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / reps, reps


def run_roi_nms(dev, reps=20, only=None):
    """``also.roi_nms`` and the top-level ``roofline_hbm``: every case of ROI_NMS_CASES in both cache states.  Per state:
    ``events_us`` (live, this run), and from the committed rocprofv3 passes of the SAME launches (profiles/r06_roi_nms_pmc.json,
    tools/roi_nms_pmc.sh: >= 100 launches per pass, the first 5 dropped) ``rocprof_us``, ``traffic`` (HBM bytes per op from the
    FETCH_SIZE / WRITE_SIZE passes, corrected as the guide prescribes) and ``frac`` = algorithmic bytes / rocprof_us / 8 TB/s
    (``frac_events`` beside it; where no rocprof record exists ``frac`` falls back to the event time and ``source`` says so)."""
    import torch
    pmc, pmc_name = {}, None
    for cand in ROI_NMS_PMC:
        path = os.path.join(ROOT, "profiles", cand)
        if os.path.exists(path):
            try:
                with open(path) as f:
                    rec = json.load(f)
                # a record of OTHER kernels (roi_ops.hip / rpn.hip edited since) is not quoted: the next older record, or -- when
                # none is current -- frac falls back to this run's events
                if record_is_current(rec):
                    pmc, pmc_name = rec.get("cases", {}), cand
                    break
            except Exception:
                continue
    out = {}
    blocker = torch.randn(8192, 8192, device=dev)
    for name in ROI_NMS_CASES:
        if only and only not in name:
            continue
        row = {"bound": "hbm", "peak": 8000.0, "unit": "GB/s"}
        for state in ("warm", "cold"):
            case = roi_nms_case(dev, name, cold=state == "cold")
            us, n = time_roi_nms_case(dev, case, blocker, reps)
            nbytes = case["nbytes"]
            st = {"events_us": us, "frac_events": nbytes / us / 1e3 / 8000.0, "sets": case["sets"], "launches_timed": n}
            p = pmc.get(name, {}).get(state)
            if p:
                st.update(rocprof_us=p["avg_us"], achieved=nbytes / p["avg_us"] / 1e3, frac=nbytes / p["avg_us"] / 1e3 / 8000.0,
                          traffic=p["hbm_bytes_corrected"], traffic_over_algorithmic=p["traffic_over_algorithmic"],
                          source="profiles/" + pmc_name)
            else:
                st.update(rocprof_us=None, achieved=nbytes / us / 1e3, frac=st["frac_events"], traffic=None,
                          source="HIP events of this run (no rocprofv3 record for this case)")
            row[state] = st
            row["algorithmic_bytes"] = nbytes
            row["kernels"] = sorted(case["kernels"])
            del case
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
        out[name] = row
    del blocker
    out["note"] = ("warm = one buffer set launched back to back (maps and outputs in the 256 MiB Infinity Cache: the op's state "
                   "inside a step); cold = a rotation over >= 512 MiB of distinct maps and outputs; events_us = one event pair "
                   "around the launches behind a blocker GEMM (includes the ~1-2 us between two launches), rocprof_us = the "
                   "kernels' own durations; NMS = mask + scan kernels on the reference algorithm's bytes (the scan is a latency "
                   "chain, not a stream)")
    return out


def roofline_hbm(roi_nms):
    """The metric's second half as a top-level object next to ``roofline`` (the driver's record keeps top-level keys only):
    the RoIAlignAvg forward at configs[2]'s size (4 frames x 32 ROIs) from HBM (cold state), with the other HBM-side ops of
    the path as numeric rows."""
    main = roi_nms.get("roi_align_avg_fwd_4x32")
    if not main or "cold" not in main:
        return None
    c = main["cold"]
    out = {"bound": "hbm", "kernel": "roi_align_fwd_roi_kernel", "case": "RoIAlignAvg forward, 4 frames x 32 ROIs, 1024 channels, cold "
           "(maps and outputs rotate over >= 512 MiB)", "achieved": c["achieved"], "peak": 8000.0, "unit": "GB/s", "frac": c["frac"],
           "traffic": c["traffic"], "algorithmic_bytes": main["algorithmic_bytes"], "rocprof_us": c["rocprof_us"],
           "events_us": c["events_us"], "frac_events": c["frac_events"], "source": c["source"], "cases": {}}
    for name, row in roi_nms.items():
        if not isinstance(row, dict) or "warm" not in row:
            continue
        for state in ("warm", "cold"):
            st = row[state]
            out["cases"]["%s.%s" % (name, state)] = {"us": st["rocprof_us"] if st["rocprof_us"] is not None else st["events_us"],
                                                     "events_us": st["events_us"], "achieved": st["achieved"], "frac": st["frac"],
                                                     "traffic": st["traffic"], "algorithmic_bytes": row["algorithmic_bytes"]}
    return out


# ----------------------------------------------------------------------------- configs[1] / configs[3]
def run_sgg(a, rank, world, dev, frames_per_rank=2):
    import torch
    from i2vsgg_amd import train
    net = train.build_sgg_net(a.layers, device=dev)
    step = train.SGGEmbStep(net, frames_per_rank, seed=1 + rank, device=dev, use_graph=not a.no_graph)
    graphed = step.capture(warmup=2)
    elapsed = timed_steps(step, a.warmup, a.steps, dev)
    keep_outputs(a, rank, lambda: dict(loss=step.loss.reshape(1), fmap=step.fmap, **param_outputs(
        [(n, p) for n, p in net.named_parameters() if n.startswith("vrd.")], cap=1 << 20)))
    loss = float(step.loss)
    tp = getattr(step, "tp", False)
    line = {
        "metric": "frames/sec (600x1000, 32 ROI/frame)", "value": world * frames_per_rank * a.steps / elapsed,
        "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": 1e3 * elapsed / a.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[%d]: cfgs/res101.yml, SGG_emb fwd+bwd+SGD, %d frames/GPU "
                               "600x1000, 32 boxes + 32 pairs/frame, ResNet-%d C4" % (3 if world > 1 else 1, frames_per_rank, a.layers),
                   "frames_per_gpu": frames_per_rank, "global_frames": world * frames_per_rank,
                   "hip_graph": bool(graphed), "graph_error": step.graph_error,
                   "parallelism": ("dp%d (frames sharded) + vrd.fc6 cut by output columns across the ranks: RCCL all-reduce of the "
                                   "other 84 MB of gradients, 30 MB of activation gathers for fc6" % world) if tp
                   else "dp%d (frames sharded, RCCL all-reduce of vrd grads)" % world,
                   "schedule": (("one graph per step: [head fwd+bwd (+ gradient exchange) + SGD of batch k] beside [stem..layer3[:%d] "
                                 "of batch k+2, both frames per launch] beside [layer3[%d:] of batch k+1]; every step = 1 backbone pass "
                                 "(its two halves on consecutive minibatches) + 1 head pass + 1 update, all inside the timed region"
                                 % (step.cut, step.cut)) if step.stage_split else
                                ("one graph per step: [head fwd+bwd (+ gradient exchange) + SGD of batch k] beside the backbone fwd "
                                 "of batch k+1 (one graph branch per frame); every step = 1 backbone pass + 1 head pass + 1 update, all "
                                 "inside the timed region")) if step.overlap
                   else "one graph per step: backbone fwd, head fwd+bwd, fused wgrad+SGD" if graphed else "eager launches",
                   "loss": loss},
    }
    if a.full:
        line["roofline"] = sgg_roofline(a, rank, dev, step, elapsed)
    return line, step, net


def sgg_roofline(a, rank, dev, step, elapsed):
    """--full: the roofline block of the relation step, from eager steps of the same objects profiled with HIP events."""
    import re
    # ---- roofline of the dominant kernel: conv_igemm_f32 (MFMA-bound)
    n_prof = 3
    pp, step._pipelined = step._pipelined, False          # the profiled steps are sequential eager steps of the same objects
    rec = profile_eager(step._body, n_prof, dev)
    step._pipelined = pp
    # The dominant kernel of the step is conv_gemm_f32 (the pointwise layers of the bottlenecks: 60 of the ~110 GEMM launches
    # and most of the conv time): every call tagged [gemm] is exactly one launch of it, so flops / HIP-event time of those
    # calls is the kernel's own rate.  `all_conv` keeps the whole-backbone view (every i2v_conv_fwd / convolution _dgrad
    # call, Winograd transform kernels included in the time): executed MACs (Winograd F(4x4,3x3) runs 1/4 of the direct
    # count, F(2x2) 4/9) and the direct convolution's algorithmic count.
    gemm = [r for r in rec if r["tag"] == "fwd" and "[gemm]" in r["desc"]]
    t_gemm = sum(r["t"] for r in gemm)
    f_gemm = sum(r["flops"] for r in gemm)
    b_gemm = sum(r["bytes"] for r in gemm)
    n_gemm = max(len(gemm) // n_prof, 1)
    conv = [r for r in rec if r["tag"] in ("fwd", "dgrad") and "(wgrad form)" not in r["desc"]]
    t_conv = sum(r["t"] for r in conv)
    f_alg = sum(r["flops"] for r in conv)
    f_exec = sum(r["flops"] * (0.25 if "winograd F4" in r["desc"] else 4.0 / 9.0 if "winograd" in r["desc"] else 1.0) for r in conv)
    if a.dump_launches and rank == 0:
        per = len(rec) // n_prof
        with open(a.dump_launches, "w") as f:
            for r in rec[-per:]:
                f.write("%-6s %-52s %8.1f us %7.2f GF %6.1f TF %8.2f MB\n" % (
                    r["tag"], r["desc"], r["t"] * 1e6, r["flops"] / 1e9, r["flops"] / r["t"] / 1e12, r["bytes"] / 1e6))
    traffic, traffic_src = pmc_traffic("conv_gemm_f32")
    achieved = f_gemm / max(t_gemm, 1e-12) / 1e12
    # algorithmic bytes of EVERY conv_gemm_f32 launch of a step, for the comparison with the PMC traffic (which averages over
    # all launches of the kernel): the pointwise calls + the batched plane GEMM inside every Winograd call
    wino = [r for r in rec if "winograd" in r["desc"] and "gemmMB=" in r["desc"]]
    b_wino = sum(float(re.search(r"gemmMB=([0-9.]+)", r["desc"]).group(1)) * 1e6 for r in wino)
    n_all = max((len(gemm) + len(wino)) // n_prof, 1)
    b_all = (b_gemm + b_wino) / n_prof / n_all
    roof = {"bound": "mfma", "kernel": "conv_gemm_f32 (pointwise bottleneck layers and the other plain GEMMs it serves; one "
                                       "launch per call)",
            "achieved": achieved, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": achieved / MFMA_F32_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_src,
            "note": ("achieved = 2*M*N*K of every conv_gemm_f32 launch of a step / the summed launch durations (HIP events "
                     "on the launch stream around every call of %d eager steps of the same objects); all MACs are "
                     "executed MACs.  all_conv = every convolution forward / data-gradient call of the step "
                     "(Winograd layers included with their transform kernels)") % n_prof,
            "launches_per_step": n_gemm, "avg_launch_us": 1e6 * t_gemm / max(len(gemm), 1),
            "algorithmic_bytes_per_launch": b_all, "launches_per_step_incl_winograd_planes": n_all,
            "traffic_over_algorithmic": (traffic / b_all) if traffic else None,
            "algorithmic_bytes_per_pointwise_launch": b_gemm / n_prof / n_gemm,
            "gflop_per_step": f_gemm / n_prof / 1e9,
            "all_conv": {"ms_per_step": 1e3 * t_conv / n_prof, "launches_per_step": len(conv) // n_prof,
                         "executed_tflops": f_exec / t_conv / 1e12,
                         "executed_frac": f_exec / t_conv / 1e12 / MFMA_F32_PEAK_TFLOPS,
                         "algorithmic_tflops": f_alg / t_conv / 1e12,
                         "algorithmic_frac": f_alg / t_conv / 1e12 / MFMA_F32_PEAK_TFLOPS,
                         "gflop_executed_per_step": f_exec / n_prof / 1e9,
                         "gflop_algorithmic_per_step": f_alg / n_prof / 1e9},
            "by_kind": by_kind(rec, n_prof)}
    # the whole step against the matrix pipe: every GEMM-shaped launch of a step (backbone, head forward, data and filter
    # gradients, fused updates), executed MACs (Winograd F(4x4,3x3) runs 1/4 of the direct count) / the TIMED ms per step
    wf = lambda r: 0.25 if "winograd F4" in r["desc"] else 4.0 / 9.0 if "winograd" in r["desc"] else 1.0   # noqa: E731
    g_exec = sum(r["flops"] * wf(r) for r in rec) / n_prof / 1e9
    g_alg = sum(r["flops"] for r in rec) / n_prof / 1e9
    ms = 1e3 * elapsed / a.steps
    roof["step"] = {"gflop_executed_per_step": g_exec, "gflop_algorithmic_per_step": g_alg, "ms_per_step": ms,
                    "executed_tflops": g_exec / ms, "frac": g_exec / ms / MFMA_F32_PEAK_TFLOPS,
                    "algorithmic_frac": g_alg / ms / MFMA_F32_PEAK_TFLOPS,
                    "note": "every GEMM-shaped launch of one step / the timed ms per step of the replayed graph; the "
                            "fc6 path (forward 0.43 ms + fused update 0.79 ms of kernel time for 4.1 GB) is HBM-bound, "
                            "not MFMA-bound: profiles/r05_step_budget.txt has the per-kind budget"}
    return roof


# ----------------------------------------------------------------------------- configs[1] fed by the data layer
def run_sgg_loader(a, rank, world, dev, frames_per_rank=2, n_batches=8, u8=False):
    """The same step fed as the reference loop is fed (trainval_net_SGG_emb.py:77-91,204-217): combined_roidb ->
    roibatchLoader(path_return=True) -> DataLoader(sampler) on a synthetic imdb whose frames come in five resolutions with
    4-32 boxes and 2-32 annotated pairs each.  ``n_batches`` collated minibatches are kept in pinned host memory (the loader's
    own CPU time -- synthetic pixels, the host resize -- is reported separately: its workers run beside the GPU); every
    timed step stages one of them (frames and packed head inputs cross PCIe, pair tables are built on the host) and replays
    the captured step of that minibatch's size."""
    import torch
    from i2vsgg_amd import train
    from i2vsgg_amd.model.utils import config as c
    from i2vsgg_amd.model.utils.net_utils import sampler
    from i2vsgg_amd.roi_data_layer.roibatchLoader import collate_device_prep, roibatchLoader
    from i2vsgg_amd.roi_data_layer.roidb import combined_roidb
    c.cfg.TRAIN.USE_FLIPPED = False
    imdb, roidb, ratio_list, ratio_index = combined_roidb("synthetic_%d_v" % (2 * n_batches * frames_per_rank * world))
    # u8: the device front-end form of the loader (uint8 frames as decoded; BGR swap, mean subtraction, resize and canvas
    # placement by i2v_image_prep inside the timed region)
    ds = roibatchLoader(roidb, ratio_list, ratio_index, frames_per_rank, imdb.num_classes, training=True, path_return=True,
                        device_prep=u8)
    dl = torch.utils.data.DataLoader(ds, batch_size=frames_per_rank, pin_memory=True, collate_fn=collate_device_prep if u8 else None,
                                     sampler=sampler(len(roidb), frames_per_rank, rank=rank, world=world, seed=c.cfg.RNG_SEED))
    t0 = time.perf_counter()
    batches = []
    for d in dl:
        if u8 and (not isinstance(d, list) or int(d[1][0][1]) <= 0):
            continue                      # a square-trim minibatch goes through the host form in a training loop
        batches.append(d)
        if len(batches) == n_batches:
            break
    loader_ms = 1e3 * (time.perf_counter() - t0) / len(batches)
    net = train.build_sgg_net(a.layers, device=dev)
    net.vrd.source_gt_rels = imdb.gt_rels(net.vrd.n_rel)
    step = train.SGGEmbStep(net, frames_per_rank, device=dev, use_graph=not a.no_graph, stage_synthetic=False)
    hw = (lambda d: (int(d[1][0][1]), int(d[1][0][2]))) if u8 else (lambda d: (int(d[0].shape[2]), int(d[0].shape[3])))
    stage = step.stage_batch_u8 if u8 else step.stage_batch
    for d in batches:                     # the feature-map buffers fit the largest minibatch from the start
        step.reserve(*hw(d))
    assert stage(batches[0])
    graphed = step.capture(warmup=2)
    pos = [0]

    def fn():
        pos[0] += 1
        stage(batches[pos[0] % len(batches)])
        step()
    for _ in range(len(batches) + 3):     # every frame size (backbone cut by stage: every pair of consecutive sizes) met once: its
        fn()                              # graph is captured outside the timed region
    bubbles = step.n_bubbles
    elapsed = timed_steps(fn, a.warmup, a.steps, dev)
    assert step.n_bubbles == bubbles, "a timed call ran no head"
    keep_outputs(a, rank, lambda: dict(loss=step.loss.reshape(1), fmap=step.fmap, **param_outputs(
        [(n, p) for n, p in net.named_parameters() if n.startswith("vrd.")], cap=1 << 20)))
    sizes = sorted({hw(d) for d in batches})
    # --full: the same graphs with their minibatch RESIDENT (staged once, replayed): what the loader-fed step would take if staging
    # cost nothing -- the loader's frames are not 600x1000 (five resolutions, 460-640 kpixel), so the headline's resident step is
    # not the yardstick.  Mean over the minibatches in the order the timed loop visits them.
    res_ms = {}
    if a.full:
        for d in batches:
            if hw(d) in res_ms:
                continue
            stage(d)
            for _ in range(1 + step.lag):     # the pipeline holds only this minibatch from here on
                step()
            res_ms[hw(d)] = 1e3 * timed_steps(step, 2, max(a.steps // 2, 5), dev) / max(a.steps // 2, 5)
    rels = net.vrd.source_gt_rels
    nb = [sum(len(rels[p.split("/")[-1]]["boxes"]) for p in d[4]) for d in batches]
    line = {
        "metric": "frames/sec (600x1000, 32 ROI/frame)", "value": world * frames_per_rank * a.steps / elapsed,
        "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": ("loader: %d collated roibatchLoader minibatches in pinned host memory, one staged per step (H2D of the frames "
                 "and the packed head inputs inside the timed region)" % len(batches)) if not u8 else
                ("loader, device front-end: %d roibatchLoader(device_prep=True) minibatches (uint8 frames as decoded) in pinned host "
                 "memory, one staged per step: H2D of the uint8 frames, BGR swap / mean subtraction / resize / canvas placement on "
                 "the device (i2v_image_prep) and the packed head inputs inside the timed region" % len(batches)),
        "config": {"workload": "BASELINE.json configs[%d] fed by roi_data_layer: cfgs/res101.yml, SGG_emb fwd+bwd+SGD, %d frames/GPU, "
                               "shorter side 600, minibatch sizes %s, %d-%d boxes per minibatch, ResNet-%d C4" % (
                                   3 if world > 1 else 1, frames_per_rank, sizes, min(nb), max(nb), a.layers),
                   "frames_per_gpu": frames_per_rank, "hip_graph": bool(graphed), "graph_error": step.graph_error,
                   "graphs": sum(1 for fs in step.shapes.values() if fs.graph), "frame_sizes": sizes,
                   "head_capacity_rows": [step.cap_boxes, step.cap_pairs],
                   "loader_cpu_ms_per_minibatch": loader_ms, "loss": float(step.loss)},
    }
    if a.full:
        resident_same = sum(res_ms[hw(d)] for d in batches) / len(batches)
        line["config"].update(resident_ms_per_step_at_these_sizes=resident_same,
                              resident_ms_by_size={"%dx%d" % k: v for k, v in sorted(res_ms.items())},
                              staging_cost_ms_per_step=1e3 * elapsed / a.steps - resident_same)
    return line, step, net


# ----------------------------------------------------------------------------- the test loops
def run_eval(a, dev, frames=4, n_iter=24, n_boxes=8):
    import torch
    from i2vsgg_amd import eval as ev, synthetic as syn, train
    ims = [torch.from_numpy(syn.frames(100 + i, 1)[0]).to(dev).contiguous(memory_format=torch.channels_last) for i in range(4)]
    info = torch.tensor([[600.0, 1000.0, 1.0]], device=dev)
    z, nb = torch.zeros(1, 1, 5, device=dev), torch.zeros(1, device=dev)

    def per_frame(fn, n):
        fn(0); fn(1)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        for i in range(n):
            fn(2 + i)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) / n

    def stepped(step, batches):
        for b in batches[:2]:
            step(*b)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        n = sum(len(r) for r in step.run(batches[i % len(batches)] for i in range(n_iter // frames)))
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) / n

    out = {"unit": "frames/s", "frames_in_flight": frames, "frame": "600x1000 synthetic, ResNet-%d" % a.layers}
    det = train.build_instance_styled_net(a.layers, device=dev).eval()
    t0 = per_frame(lambda i: ev.detect_frame(det, ims[i % 4], info, z, nb), n_iter)
    step = ev.DetectStep(det, frames=frames, device=dev, use_graph=not a.no_graph)
    t1 = stepped(step, [(torch.cat([ims[(i + j) % 4] for j in range(frames)]), info.expand(frames, 3).contiguous()) for i in range(4)])
    out["detect"] = {"loop": "test_net_instance_styleD_bilinear.py:133-221 (TEST: 6000 -> 300 proposals, 16 classes, NMS 0.3, top 100)",
                     "frame_by_frame": 1.0 / t0, "graph_step": 1.0 / t1, "hip_graph": bool(step.shapes[step._staged].graph),
                     "graph_error": step.graph_error}
    del step, det
    torch.cuda.empty_cache()
    sgg = train.build_sgg_net(a.layers, device=dev).eval()
    sgg.vrd.target_gt_rels = {"f%d" % i: syn.relation_annotation(31 + i, n_boxes, n_boxes, 62, 16) for i in range(4)}
    t0 = per_frame(lambda i: ev.relation_frame(sgg, ims[i % 4], info, "f%d" % (i % 4)), n_iter)
    step = ev.RelationStep(sgg, frames=frames, device=dev, cap_boxes=n_boxes + 1, use_graph=not a.no_graph)
    t1 = stepped(step, [(torch.cat([ims[(i + j) % 4] for j in range(frames)]), info.expand(frames, 3).cpu().numpy(),
                         ["f%d" % ((i + j) % 4) for j in range(frames)]) for i in range(4)])
    out["relation"] = {"loop": "test_net_SGG_emb.py per frame (%d annotated boxes, %d ordered pairs, top-100 triplets)" % (
                           n_boxes, n_boxes * (n_boxes - 1)),
                       "frame_by_frame": 1.0 / t0, "graph_step": 1.0 / t1, "hip_graph": bool(step.shapes[step._staged].graph),
                       "graph_error": step.graph_error}
    return out


# ----------------------------------------------------------------------------- configs[2]
def run_instance_styled(a, rank, world, dev, steps, warmup, frames_per_rank=4):
    import numpy as np
    import torch
    from i2vsgg_amd import train
    from i2vsgg_amd.model.utils import config as c
    np.random.seed(c.cfg.RNG_SEED + rank)
    net = train.build_instance_styled_net(a.layers, device=dev)
    step = train.InstanceStyleDStep(net, frames_per_rank, seed=3 + rank, device=dev)
    graphed = step.capture(warmup=2) if (hasattr(step, "capture") and not a.no_graph) else False
    if not graphed:
        for _ in range(2):
            step()
    elapsed = timed_steps(step, warmup, steps, dev)
    keep_outputs(a, rank, lambda: dict({"loss." + k: torch.as_tensor(v).reshape(1) for k, v in step.losses.items()},
                                       **param_outputs(net.named_parameters(), budget=6 << 20)))
    losses = {k: float(v) for k, v in step.losses.items()}
    roof = isd_roofline(a, rank, dev, step) if a.full else None
    line = {
        "metric": "frames/sec (600x1000, 32 ROI/frame)", "value": world * 2 * frames_per_rank * steps / elapsed,
        "unit": "frames/s", "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[2]: cfgs/res101.yml, instance_styleD D+G adversarial step, %d source + %d "
                               "target frames/GPU 600x1000, 32 ROI/frame, ResNet-%d, layer1-3 + heads trained" % (
                                   frames_per_rank, frames_per_rank, a.layers),
                   "frames_per_gpu": 2 * frames_per_rank, "hip_graph": bool(graphed),
                   "graph_error": getattr(step, "graph_error", None),
                   "parallelism": "dp%d (frames sharded, RCCL all-reduce of 202 MB of gradients)" % world,
                   "losses": losses, "max_mem_GB": torch.cuda.max_memory_allocated(dev) / 2 ** 30},
    }
    if roof is not None:
        line["roofline"] = roof
    return line, step, net


def isd_roofline(a, rank, dev, step):
    """--full: the roofline block of the configs[2] step, from eager steps of the same objects profiled with HIP events."""
    n_prof = 2
    rec = profile_eager(step.eager_step if hasattr(step, "eager_step") else step, n_prof, dev)
    if a.dump_launches and rank == 0:
        per = len(rec) // n_prof
        with open(a.dump_launches, "w") as f:
            for r in rec[-per:]:
                f.write("%-6s %-52s %8.1f us %7.2f GF %6.1f TF %8.2f MB\n" % (
                    r["tag"], r["desc"], r["t"] * 1e6, r["flops"] / 1e9, r["flops"] / r["t"] / 1e12, r["bytes"] / 1e6))
    wg = [r for r in rec if r["tag"] == "wgrad"]
    t_wg, f_wg, b_wg = sum(r["t"] for r in wg), sum(r["flops"] for r in wg), sum(r["bytes"] for r in wg)
    # the 3x3 layers' filter gradients run in the Winograd F(4x4,3x3) domain: a quarter of the direct form's MACs are
    # executed (plus transforms).  `achieved` counts EXECUTED MACs (what the matrix pipe did); the direct-convolution
    # count is reported beside it
    f_wg_exec = sum(r["flops"] * (0.25 if "winograd F4" in r["desc"] else 1.0) for r in wg)
    achieved = f_wg_exec / max(t_wg, 1e-12) / 1e12
    # the PMC passes of THIS configuration (tools/profile_bench.sh isd), not the headline's (whose conv_wgrad2_f32 launches
    # are the relation head's skinny GEMMs)
    traffic, traffic_src = pmc_traffic("conv_wgrad2_f32", ("r06_instance_styled_pmc_summary.json", "r05_instance_styled_pmc_summary.json", "r04_instance_styled_pmc_summary.json", "r03_instance_styled_pmc_summary.json", "r02_instance_styled_pmc_summary.json"))
    return {"bound": "mfma", "kernel": "conv_wgrad2_f32 (every filter gradient of the step; executed MACs, the "
                                       "Winograd-domain 3x3 layers included with their transform kernels)", "achieved": achieved,
            "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / MFMA_F32_PEAK_TFLOPS,
            "algorithmic_tflops": f_wg / max(t_wg, 1e-12) / 1e12,
            "traffic": traffic, "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": b_wg / max(len(wg), 1), "launches_per_step": len(wg) // n_prof,
            "avg_launch_us": 1e6 * t_wg / max(len(wg), 1), "by_kind": by_kind(rec, n_prof)}


# ----------------------------------------------------------------------------- configs[4]
def run_joint(a, rank, world, dev, frames_per_rank=4):
    """One instance_styleD D+G step followed by one SGG_emb step on the same number of frames."""
    import numpy as np
    import torch
    from i2vsgg_amd import train
    from i2vsgg_amd.model.utils import config as c
    np.random.seed(c.cfg.RNG_SEED + rank)
    det = train.build_instance_styled_net(a.layers, device=dev)
    dstep = train.InstanceStyleDStep(det, frames_per_rank, seed=3 + rank, device=dev)
    dgraph = dstep.capture(warmup=2) if (hasattr(dstep, "capture") and not a.no_graph) else False
    sgg = train.build_sgg_net(a.layers, device=dev)
    sstep = train.SGGEmbStep(sgg, frames_per_rank, seed=1 + rank, device=dev, use_graph=not a.no_graph)
    sgraph = sstep.capture(warmup=2)

    def both():
        dstep()
        sstep()
    elapsed = timed_steps(both, a.warmup, a.steps, dev)
    keep_outputs(a, rank, lambda: {
        **{"det.loss." + k: torch.as_tensor(v).reshape(1) for k, v in dstep.losses.items()}, "sgg.loss": sstep.loss.reshape(1),
        **param_outputs([("det." + n, p) for n, p in det.named_parameters()], budget=4 << 20),
        **param_outputs([("sgg." + n, p) for n, p in sgg.named_parameters() if n.startswith("vrd.")], budget=2 << 20)})
    roof = joint_roofline(dev, dstep, sstep) if a.full else None
    line = {
        "metric": "frames/sec (600x1000, 32 ROI/frame)", "value": world * frames_per_rank * a.steps / elapsed,
        "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[4]: joint instance_styleD D+G step (%d source + %d target frames/GPU) + "
                               "SGG_emb step on %d frames/GPU, 600x1000, 32 ROI/frame; a frame counts once" % (
                                   frames_per_rank, frames_per_rank, frames_per_rank),
                   "frames_per_gpu": frames_per_rank, "hip_graph": [bool(dgraph), bool(sgraph)],
                   "parallelism": "dp%d (RCCL all-reduce of 202 MB + the vrd gradients)" % world,
                   "loss_sgg": float(sstep.loss), "loss_det": float(dstep.losses["total"]),
                   "losses_det": {k: float(v) for k, v in dstep.losses.items()},
                   "max_mem_GB": torch.cuda.max_memory_allocated(dev) / 2 ** 30},
    }
    if roof is not None:
        line["roofline"] = roof
    return line, (dstep, sstep), (det, sgg)


def joint_roofline(dev, dstep, sstep):
    """--full: the roofline block of the joint step.  The dominant kernel: every conv_gemm_f32 launch of both halves (the
    pointwise layers of the detector's trained trunk, forward and data gradient, and of the relation net's frozen trunk), HIP
    events around every call of eager steps of the same objects."""
    n_prof = 2
    pp, sstep._pipelined = sstep._pipelined, False

    def eager_both():
        dstep.eager_step()
        sstep._body()
    rec = profile_eager(eager_both, n_prof, dev)
    sstep._pipelined = pp
    gemm = [r for r in rec if r["tag"] in ("fwd", "dgrad") and ("[gemm]" in r["desc"] or "+epi" in r["desc"]) and "winograd" not in r["desc"]]
    t_gemm, f_gemm = sum(r["t"] for r in gemm), sum(r["flops"] for r in gemm)
    achieved = f_gemm / max(t_gemm, 1e-12) / 1e12
    return {"bound": "mfma", "kernel": "conv_gemm_f32 / conv_igemm_f32 pointwise launches of both halves (forward and fused data "
                                       "gradient of the 1x1 layers; one launch per call)",
            "achieved": achieved, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / MFMA_F32_PEAK_TFLOPS,
            "traffic": None, "launches_per_step": len(gemm) // n_prof, "avg_launch_us": 1e6 * t_gemm / max(len(gemm), 1),
            "gflop_per_step": f_gemm / n_prof / 1e9, "by_kind": by_kind(rec, n_prof),
            "note": "2*M*N*K of the launches / their summed durations (HIP events on the launch stream, %d eager joint "
                    "steps of the same objects); the timed region replays the two captured graphs" % n_prof}


# ----------------------------------------------------------------------------- configs[0]
def run_res50(a, rank, world, dev):
    """cfgs/res50.yml, ONE 1x3x600x1000 frame: Faster-RCNN (instance_styleD detector, eval) forward + SGG_emb relation head
    forward on the same frame -- the reference's CPU-runnable plumbing case; here timed on the GPU."""
    import torch
    from i2vsgg_amd import train, synthetic as syn
    from i2vsgg_amd.model.utils import config as c
    det = train.build_instance_styled_net(50, device=dev).eval()
    sgg = train.build_sgg_net(50, device=dev).eval()
    im, info = syn.frames(0, 1, 600, 1000)
    gt, nb = syn.gt_boxes(0, 1, 8, det.n_classes, c.cfg.MAX_NUM_GT_BOXES, 600, 1000)
    to = lambda x: torch.from_numpy(x).to(dev)
    imd, infod, gtd, nbd = to(im), to(info), to(gt), to(nb)
    sstep = train.SGGEmbStep(sgg, 1, seed=0, device=dev, n_boxes=8, n_pairs=8, use_graph=False)

    last = []

    def fwd():
        with torch.no_grad():
            out = det(imd, infod, gtd, nbd)
            fmap = sgg.RCNN_base(sstep.im)
            score, _ = sgg.vrd.forward_device(fmap, sstep.boxes, sstep.relb, sstep.masks, sstep.ixs, sstep.ixo)
        last[:] = [out, score]
        return out, score
    elapsed = timed_steps(fwd, a.warmup, a.steps, dev)
    names = ("rois", "cls_prob", "bbox_pred")          # the detector's eval outputs (faster_rcnn_instance_styleD_bilinear.py)
    keep_outputs(a, rank, lambda: dict({(names[i] if i < len(names) else "det_out%d" % i): (t, 1 << 20)
                                        for i, t in enumerate(last[0]) if torch.is_tensor(t)}, rel_score=last[1]))
    out, score = fwd()
    line = {
        "metric": "frames/sec (600x1000, 32 ROI/frame)", "value": world * a.steps / elapsed, "unit": "frames/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[0]: cfgs/res50.yml, 1x3x600x1000, Faster-RCNN forward (RPN_BATCHSIZE %d, %d "
                               "test proposals) + SGG_emb head forward (8 boxes, 8 pairs), eager" % (
                                   c.cfg.TRAIN.RPN_BATCHSIZE, out[0].shape[1]),
                   "frames_per_gpu": 1, "hip_graph": False, "rois": list(out[0].shape), "rel_score": list(score.shape)},
    }
    return line, sstep, (det, sgg)


# ----------------------------------------------------------------------------- main
def dry_run(a):
    """Launcher rehearsal without a GPU: rendezvous over gloo on 127.0.0.1, one collective, the JSON line."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if os.environ.get("I2V_BENCH_FAIL_RANK") == str(rank):      # tests: a rank that never comes up
        sys.exit(7)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)])
    if world > 1:
        dist.all_reduce(t)
    if int(t.item()) != world * (world + 1) // 2:
        sys.exit(3)
    if rank == 0:
        print(json.dumps({"metric": "frames/sec (600x1000, 32 ROI/frame)", "value": 0.0, "unit": "frames/s", "n_gpus": world,
                          "steps": a.steps, "warmup": a.warmup, "dry_run": True, "config": {"workload": a.config}}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ:
        launch_ranks(a.gpus)                 # does not return
    if a.dry_run:
        return dry_run(a)

    import torch
    from i2vsgg_amd import parallel
    from i2vsgg_amd.model.utils import config as c
    rank, world, dev = parallel.init_from_env()
    assert dev.type == "cuda", "bench.py needs a GPU (the product path has no CPU fallback)"
    if world != a.gpus:
        sys.stderr.write("bench.py: --gpus %d but the process group has %d ranks\n" % (a.gpus, world))
        sys.exit(2)
    c.cfg_from_file(c.default_cfg_file("res50" if a.config == "res50" else "res101"))
    c.cfg_from_list(SET_CFGS)

    keep = []
    if a.config == "sgg" and a.data in ("loader", "loader_u8"):
        line, step, net = run_sgg_loader(a, rank, world, dev, u8=a.data == "loader_u8")
        keep += [step, net]
    elif a.config == "sgg":
        line, step, net = run_sgg(a, rank, world, dev)
        keep += [step, net]
        if world == 1 and a.full and not a.no_also:
            # Secondary measurements under the same driver clock.  Each is guarded: whatever happens in one of them, the headline
            # line above is printed (a failure is recorded under "also" with its message).
            line["also"] = {}
            pick = lambda ld: {k: ld[k] for k in ("value", "unit", "ms_per_step", "steps", "data", "config")}
            sub = argparse.Namespace(**dict(vars(a), dump_outputs=""))      # --dump-outputs holds the headline's outputs

            def also(name, fn):
                try:
                    line["also"][name] = fn()
                except Exception as e:      # noqa: BLE001 -- the message goes into the line
                    line["also"][name] = {"error": repr(e)[:400]}
                torch.cuda.synchronize(dev)
                torch.cuda.empty_cache()

            def loader(u8):
                # the same step fed by the data layer (varying minibatch sizes, staged from the host every step)
                ld, s1, n1 = run_sgg_loader(sub, rank, world, dev, u8=u8)
                s1.opt.unfuse()
                return pick(ld)


            def isd():
                # configs[2]: fewer steps (a step is ~10x longer), its own roofline block
                res, s2, n2 = run_instance_styled(sub, rank, world, dev, steps=max(4, a.steps // 4), warmup=2)
                return res

            def eval_loops():
                # the two TEST loops (test_net_instance_styleD_bilinear.py:133-221, test_net_SGG_emb.py per frame) on 600x1000
                # frames: frame by frame as the reference evaluates (eval.detect_frame / relation_frame, eager launches) and as
                # replayed graphs with a branch per frame (eval.DetectStep / RelationStep, 4 frames in flight, host unpacking of
                # one batch under the next); results are bit-equal (tests/test_gpu_models.py)
                return run_eval(a, dev)

            step.opt.unfuse()
            torch.cuda.empty_cache()
            also("sgg_loader", lambda: loader(False))
            also("sgg_loader_u8", lambda: loader(True))
            also("roi_nms", lambda: run_roi_nms(dev))
            if "error" not in line["also"]["roi_nms"]:
                line["roofline_hbm"] = roofline_hbm(line["also"]["roi_nms"])
            also("instance_styled", isd)
            also("eval_loops", eval_loops)
    elif a.config == "instance_styled":
        line, step, net = run_instance_styled(a, rank, world, dev, a.steps, a.warmup)
        keep += [step, net]
    elif a.config == "joint":
        line, step, net = run_joint(a, rank, world, dev)
        keep += [step, net]
    else:
        line, step, net = run_res50(a, rank, world, dev)
        keep += [step, net]

    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline and a.config == "sgg":
        # the GPU box grants a CPU share (16 cores per GPU), not the whole host: never oversubscribe
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        threads = min(16, cores)
        second = 8 if threads > 8 else max(1, threads // 2)       # a second run at half the threads
        sec = cpu_baseline([threads, second] if second != threads else [threads])
        try:
            stages = cpu_baseline_stages(threads)
        except Exception as e:              # noqa: BLE001 -- the end-to-end figure above stands on its own
            stages = {"error": repr(e)[:400]}
        line["cpu_baseline"] = {"value": 1.0 / sec[threads], "unit": "frames/s", "cores": threads, "threads": threads, "kind": "port",
                                "by_threads": {str(t): {"frames_per_s": 1.0 / v, "s_per_frame": v} for t, v in sec.items()},
                                "sample": "1 frame 600x1000: ResNet-101 C4 fwd + vrd head fwd/bwd/SGD for 32 boxes + 32 pairs; 2 "
                                          "warm-up + 5 timed, median %.2f s" % sec[threads],
                                "stages": stages,
                                "stages_sample": "the oracle stage by stage on ONE 600x1000 frame / 32 ROIs, same protocol; "
                                                 "instance_styled_dg_step_1+1_frames = the configs[2] D+G step (fwd, bwd, SGD) on 1 "
                                                 "source + 1 target frame, 1 warm-up + 2 timed; vrd_head_fwd_bwd 1 + 3 (frames_per_s counts both frames)"}
    if rank == 0 and a.dump_outputs:
        write_outputs(a.dump_outputs)
    if rank == 0:
        print(json.dumps(line), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        # the graphs that captured RCCL kernels go first: tearing the communicator down under them can abort
        import gc
        torch.cuda.synchronize(dev)
        for obj in keep:
            opt = getattr(obj, "opt", None)
            if opt is not None:
                opt.unfuse()
        del keep, step, net
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
