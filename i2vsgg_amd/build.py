"""Build libi2vsgg_hip.so (gfx950) in-tree with hipcc.  hipcc cross-compiles without a GPU."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libi2vsgg_hip.so")
SOURCES = ["api.cpp", "roi_ops.hip", "rpn.hip", "sort.hip", "nms.hip", "soft_nms.hip", "det_post.hip", "conv.hip", "wgrad.hip", "elementwise.hip", "heads.hip",
           "image.hip", "winograd.hip", "dstyle.hip", "video.hip", "video_nms.hip", "det_eval.hip", "seqnms.hip", "track_stitch.hip", "recognition.hip", "relation_targets.hip",
           "image_relations.hip", "relation_features.hip", "proposal_eval.hip"]
# -ffp-contract=off: box / IoU / ROIAlign arithmetic must round once per operation like the
# reference's CPU path (no FMA contraction), or NMS threshold decisions can flip.
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-Wno-unused-value", "-Wno-unused-result"]
# MFMA accumulators in VGPRs, not AGPRs: measured on MI355X (tools/micro/mfma_rate.hip, tools/conv_ablate.py) a
# back-to-back v_mfma_f32_16x16x4_f32 stream issues every 32 cycles with VGPR accumulators but only every ~45
# cycles in the AGPR form hipcc picks by default for these kernels.
# The files with MFMA kernels get the flag (elementwise.hip has none: its kernels assemble to the same instructions either way).
EXTRA = {src: ["-mllvm", "-amdgpu-mfma-vgpr-form"] for src in ("conv.hip", "wgrad.hip", "dstyle.hip")}


STAMP = os.path.join(HERE, "build", "stamp.json")
LAST = {"mode": None}       # "compiled" / "reused" after build(): what the last call did (the driver's build check reads it)


def _digest():
    """sha256 over every source, the header, the flags and this file: a shipped .so is reused only if it was built
    from exactly these bytes (mtimes say nothing after a checkout or a copy to another box)."""
    import hashlib
    h = hashlib.sha256()
    deps = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + [os.path.join(HERE, "..", "include", "i2vsgg_hip.h"),
                                                                       os.path.abspath(__file__)]
    h.update(" ".join(FLAGS + SOURCES).encode())
    for d in deps:
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def source_digests(files):
    """{file: sha256[:16]} of kernel sources under csrc/: what a committed rocprofv3 summary records about the library it
    measured, and what bench.py compares before it quotes the summary (a record of other kernels is not quoted)."""
    import hashlib
    out = {}
    for f in files:
        with open(os.path.join(CSRC, f), "rb") as fh:
            out[f] = hashlib.sha256(fh.read()).hexdigest()[:16]
    return out


def _stale(digest):
    if not os.path.exists(OUT) or not os.path.exists(STAMP):
        return True
    try:
        import json
        with open(STAMP) as f:
            st = json.load(f)
        return st.get("digest") != digest or st.get("so_size") != os.path.getsize(OUT)
    except Exception:
        return True


def build(force=False, verbose=False):
    digest = _digest()
    if not force and not _stale(digest):
        LAST["mode"] = "reused"
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        if not os.path.exists(path):
            raise RuntimeError("source %s named in SOURCES does not exist" % path)
        obj = os.path.join(objdir, src.rsplit(".", 1)[0] + ".o")
        objs.append(obj)
        cmd = [hipcc] + FLAGS + EXTRA.get(src, []) + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", path, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError("hipcc failed on %s" % src)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs)
    import json
    with open(STAMP, "w") as f:
        json.dump({"digest": digest, "so_size": os.path.getsize(OUT)}, f)
    LAST["mode"] = "compiled"
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
