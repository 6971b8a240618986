"""Which library entries a conv / linear / bottleneck layer calls, recorded without running them.

``tracing()`` puts a recording proxy in place of ``ops.lib``.  Pure host queries (``*_bytes``, ``*_plan``, ``i2v_conv_fwd_splits``,
the tuning keys) reach the real library; every launch entry is recorded as ``[name, argument, ...]`` and -- unless
``passthrough`` -- returns 0 without being called.  An argument is recorded by its type in ``_lib.SIGNATURES``: an integer or a
float as its value, a pointer as "ptr" / "null", a buffer size as "size" (scratch buffers grow with a process's history); the
trailing stream handle is dropped.  Without ``passthrough`` the GPU check, the stream and the launch resources are CPU
stand-ins, so a layer's forward and backward run on CPU tensors in milliseconds and compute nothing.

``run_layer`` runs one row's layer (``inputs``: shapes, epilogue operands, needs, switches) forward and backward; ["backward"]
marks the border in the call list.  ``derive_route`` reads the route a layer took out of such a call list: this, run on the
commit before ``i2vsgg_amd/conv_route.py`` existed, wrote tests/golden/conv_routes.json -- never the planner.  The module touches
only names that both that commit and its successors have (``python tests/conv_trace.py recorded.json ... > table`` regenerates
the table from the inputs of recorded calls plus ``sweep_rows()``)."""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
SWITCH_DEFAULTS = dict(WINOGRAD_TRAIN=True, WINOGRAD_WGRAD=True, WINOGRAD_KEEP_V=True, WINOGRAD_TRAIN_MIN_C=64,
                       LINEAR_DGRAD_AS_WGRAD=0, SMALL_GW_BYTES=16 << 20)
HOST_QUERIES = ("i2v_conv_fwd_splits", "i2v_get_tuning", "i2v_set_tuning", "i2v_last_error", "i2v_version")
_CL = torch.channels_last


def _modules():
    from i2vsgg_amd import _lib, launch, ops
    return _lib, launch, ops


def _plain(ctype, value, _lib):
    if ctype is _lib._p:
        return "ptr" if value else "null"
    if ctype is _lib._z:
        return "size"
    return float(value) if ctype is _lib._f else int(value)


class Proxy:
    def __init__(self, real, passthrough):
        self._real, self._pass, self.calls = real, passthrough, []
        self._lib = _modules()[0]

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith("_bytes") or name.endswith("_plan") or name in HOST_QUERIES:
            return fn
        types = self._lib.SIGNATURES[name][1]
        if types and types[-1] is self._lib._p:
            types = types[:-1]              # the stream

        def entry(*args):
            self.calls.append([name] + [_plain(t, a, self._lib) for t, a in zip(types, args)])
            return fn(*args) if self._pass else 0
        return entry


class FakeArena:
    def take(self, B, C, H, W):
        return torch.zeros((B, H, W, C)).permute(0, 3, 1, 2)

    def take_flat(self, n):
        return torch.zeros((n,))


@contextlib.contextmanager
def tracing(arena=False, passthrough=False):
    """-> the proxy (``.calls``).  ``arena`` (CPU stand-ins only): the current context has a pre-zeroed arena."""
    _lib, launch, ops = _modules()
    proxy = Proxy(ops.lib, passthrough)
    patches = [(ops, "lib", proxy)]
    if not passthrough:
        split = torch.empty((launch.SplitWorkspace.BYTES,), dtype=torch.uint8)
        fake = FakeArena() if arena else None
        patches += [(ops, "_need_cuda", lambda *ts: None), (ops, "stream", lambda: 0),
                    (launch, "arena", lambda: fake), (launch, "split_buffer", lambda device=None: split),
                    (launch, "split_args", lambda device=None: (split.data_ptr(), split.numel())),
                    (launch, "workspace", lambda nbytes, device, tag="default": torch.empty((256,), dtype=torch.uint8))]
    saved = [(m, k, getattr(m, k)) for m, k, _ in patches]
    for m, k, v in patches:
        setattr(m, k, v)
    try:
        yield proxy
    finally:
        for m, k, v in saved:
            setattr(m, k, v)


@contextlib.contextmanager
def switches(values):
    ops = _modules()[2]
    saved = {k: getattr(ops, k) for k in values}
    for k, v in values.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


class _Maker:
    """Tensors of a row: uninitialised on the CPU (a trace computes nothing), seeded normal values on a device."""

    def __init__(self, device, seed):
        self.device = torch.device(device)
        self.gen = torch.Generator().manual_seed(seed)

    def __call__(self, shape, grad=False, std=1.0, positive=False):
        if self.device.type == "cpu":
            return torch.empty(tuple(shape), memory_format=_CL if len(shape) == 4 else torch.contiguous_format).requires_grad_(bool(grad))
        t = torch.randn(tuple(shape), generator=self.gen) * std
        t = (t.abs() + 0.5) if positive else t
        if len(shape) == 4:
            t = t.contiguous(memory_format=_CL)
        return t.to(self.device).requires_grad_(bool(grad))


def _grad(t):
    return None if t is None or t.grad is None else t.grad.detach()


def run_layer(kind, inputs, proxy, device="cpu", seed=0):
    """Forward and (when something needs a gradient) backward of the row's layer under ``tracing`` -> {name: tensor} of what
    it computed and the tensors it was given (``x``, ``w``, ... for a reference)."""
    ops = _modules()[2]
    mk, need = _Maker(device, seed), inputs.get("needs", {})
    fused_keys = []

    def fuse(w, on):
        if on:
            ops.FUSED_SGD[w.data_ptr()] = (torch.zeros_like(w), 1e-2, 0.9, 5e-4)
            fused_keys.append(w.data_ptr())

    with switches(inputs.get("switches", {})):
        try:
            if kind in ("conv2d", "linear"):
                x, w = mk(inputs["x"], need.get("x")), mk(inputs["w"], need.get("w"), std=0.05)
                cout = inputs["w"][0]
                fuse(w, inputs.get("fused", [False])[0])
                if kind == "linear":
                    b = mk((cout,), need.get("shift")) if inputs["bias"] else None
                    t = dict(x=x, w=w, shift=b)
                    y = ops.linear(x, w, b, inputs["relu"])
                else:
                    scale = mk((cout,), positive=True) if inputs["scale"] else None
                    shift = mk((cout,), need.get("shift")) if inputs["shift"] else None
                    t = dict(x=x, w=w, scale=scale, shift=shift)
                    B, _, H, W = inputs["x"]
                    st, pd = inputs["stride"], inputs["pad"]
                    yshape = (B, cout, (H + 2 * pd - inputs["w"][2]) // st + 1, (W + 2 * pd - inputs["w"][3]) // st + 1)
                    res = mk(yshape, need.get("res")) if inputs["res"] else None
                    if inputs.get("out"):
                        with torch.no_grad():
                            y = ops.conv2d(x, w, scale, shift, res, st, pd, inputs["relu"], out=torch.empty(yshape, device=x.device).contiguous(memory_format=_CL))
                    else:
                        y = ops.conv2d(x, w, scale, shift, res, st, pd, inputs["relu"], inputs["winograd"])
                    t["res"] = res
            elif kind == "bottleneck":
                x = mk(inputs["x"], need.get("x"))
                ws = {k: (mk(inputs[k], need.get(k), std=0.05) if inputs.get(k) else None) for k in ("w1", "w2", "w3", "wd")}
                for k, on in zip(("w1", "w2", "w3", "wd"), inputs.get("fused", [False] * 4)):
                    fuse(ws[k], on and ws[k] is not None)
                bn = {k: (mk((w.shape[0],), positive=True), mk((w.shape[0],))) for k, w in ws.items() if w is not None}
                down = (ws["wd"],) + bn["wd"] if ws["wd"] is not None else None
                t = dict(x=x, bn=bn, **ws)
                y = ops.bottleneck(x, ws["w1"], ws["w2"], ws["w3"], bn["w1"], bn["w2"], bn["w3"], down, inputs["in_relu"],
                                   inputs["out_premasked"], inputs["stride"])
            elif kind == "wgrad_raw":
                x, g = mk(inputs["x"]), mk(inputs["g"])
                return dict(x=x, g=g, gw=ops._conv_wgrad_raw(x, g, tuple(inputs["w"]), inputs["stride"], inputs["pad"]))
            elif kind == "dgrad_raw":
                g, w = mk(inputs["g"]), mk(inputs["w"], std=0.05)
                return dict(g=g, w=w, gx=ops._conv_dgrad_raw(g, w, tuple(inputs["x"]), inputs["stride"], inputs["pad"]))
            else:
                raise KeyError(kind)
            proxy.calls.append(["backward"])
            t["y"] = y.detach()
            if y.requires_grad:
                t["gy"] = mk(y.shape)
                y.backward(t["gy"])
            t.update({"g" + k: _grad(t.get(k)) for k in ("x", "w", "shift", "res", "w1", "w2", "w3", "wd")})
            return t
        finally:
            for k in fused_keys:
                ops.FUSED_SGD.pop(k, None)


def trace(kind, inputs):
    """The row's call list on CPU tensors."""
    with tracing(arena=inputs.get("arena", False)) as proxy:
        run_layer(kind, inputs, proxy)
    return proxy.calls


# ----------------------------------------------------------------------------- the route a call list shows
WGRAD_ENTRIES = {"i2v_conv_wgrad": ("direct", 13), "i2v_conv_wgrad_scaled": ("direct", 14), "i2v_conv_wgrad_sgd": ("direct", None),
                 "i2v_conv3x3_winograd4_wgrad": ("winograd_x", 10), "i2v_conv3x3_winograd4_wgrad_v": ("winograd_v", 10)}


def _placement(call):
    at = WGRAD_ENTRIES[call[0]][1]
    return None if at is None else {1.0: "arena", 0.0: "fresh"}[call[at]]


def derive_route(kind, inputs, calls):
    """(route, placement of the filter gradient or None) as the call list shows them; ``route`` is None for the raw wrappers.
    A gradient nobody needs has the route "none"; a filter whose update is fused into its gradient kernel counts as direct."""
    if kind in ("wgrad_raw", "dgrad_raw"):
        last = [c for c in calls if c[0] in WGRAD_ENTRIES]
        return None, (_placement(last[-1]) if last else None)
    cut = calls.index(["backward"])
    fwd, bwd = calls[:cut], calls[cut + 1:]
    names = [c[0] for c in fwd]
    route = dict(fwd="direct", keep_v=False, dgrad="none", dgrad_pad=0, transposed_g=False, wgrad="none", flags=0, as_linear=False)
    place = None
    if kind == "bottleneck":
        cout = inputs["w2"][0]
        if "i2v_conv3x3_winograd4_fwd_keep" in names or "i2v_conv3x3_winograd4_fwd" in names:
            route.update(fwd="winograd", keep_v="i2v_conv3x3_winograd4_fwd_keep" in names, flags=5)
        else:
            route["flags"] = [c for c in fwd if c[0] == "i2v_conv_fwd" and c[12] == 3][0][16] & ~16
        back = [c[0] for c in bwd]
        route["dgrad"] = "winograd" if "i2v_conv3x3_winograd4_dgrad" in back else "direct"
        if route["dgrad"] == "direct":
            route["dgrad_pad"] = [c for c in bwd if c[0] == "i2v_conv_dgrad_fused" and c[13] == 3][0][12] - cout
        if inputs["needs"].get("w2"):
            three = [c for c in bwd if c[0] in ("i2v_conv3x3_winograd4_wgrad", "i2v_conv3x3_winograd4_wgrad_v")
                     or (c[0] == "i2v_conv_wgrad" and c[9] == 3) or c[0] == "i2v_conv_wgrad_sgd"]
            route["wgrad"] = WGRAD_ENTRIES[three[0][0]][0]
        return route, None
    cout = inputs["w"][0]
    first = fwd[-1]
    if first[0] == "i2v_conv_fwd":
        route["flags"] = first[16] & ~16          # EPI_ZEROED is the output's placement, not the layer's epilogue
        kh = inputs["w"][2] if kind == "conv2d" else 1
        route["as_linear"] = kind == "conv2d" and kh * inputs["w"][3] > 1 and (first[12], first[13]) == (1, 1)
    else:
        keep = first[0] == "i2v_conv3x3_winograd4_fwd_keep"
        route.update(fwd="winograd", keep_v=keep, flags=(4 if first[3] == "ptr" else 8 if first[4] == "ptr" else 0) | first[12 if keep else 11])
    if bwd and bwd[0][0] == "i2v_epilogue_bwd":
        route["transposed_g"] = bwd[0][10] == "ptr"
        bwd = bwd[1:]
    if inputs["needs"].get("x") and not inputs.get("out"):
        if bwd[0][0] == "i2v_winograd4_filter_dgrad":
            assert bwd[1][0] == "i2v_conv3x3_winograd4_fwd"
            route["dgrad"], bwd = "winograd", bwd[2:]
        elif bwd[0][0] == "i2v_conv_dgrad":
            route.update(dgrad="direct", dgrad_pad=bwd[0][8] - cout)
            bwd = bwd[1:]
        else:
            assert bwd[0][0] == "i2v_conv_wgrad", bwd[0]
            route["dgrad"], bwd = "as_wgrad", bwd[1:]
    if inputs["needs"].get("w") and not inputs.get("out"):
        route["wgrad"], place = WGRAD_ENTRIES[bwd[0][0]][0], _placement(bwd[0])
        bwd = bwd[1:]
    assert not bwd, bwd
    return route, place


# ----------------------------------------------------------------------------- the synthetic sweep over the edges
def _conv(name, x, w, scale=True, shift=True, res=False, stride=1, pad=1, relu=True, winograd=True, needs=(True, True), out=False,
          sw=None, arena=False, fused=False, **extra):
    nd = dict(x=needs[0], w=needs[1], shift=bool(shift and not scale and needs[1]), res=bool(res and needs[0]))
    return dict(src="sweep", name=name, kind="conv2d",
                inputs=dict(x=list(x), w=list(w), scale=scale, shift=shift, res=res, stride=stride, pad=pad, relu=relu, winograd=winograd,
                            out=out, needs=nd, switches=sw or {}, arena=arena, fused=[fused]), **extra)


def _linear(name, m, k, n, bias=True, relu=False, needs=(True, True), sw=None, arena=False, fused=False):
    return dict(src="sweep", name=name, kind="linear",
                inputs=dict(x=[m, k], w=[n, k], bias=bias, relu=relu, needs=dict(x=needs[0], w=needs[1], shift=bool(bias and needs[1])),
                            switches=sw or {}, arena=arena, fused=[fused]))


def _block(name, cin, p1, p2, cout, down=False, stride=1, in_relu=False, premasked=False, needs=(True,) * 5, sw=None, arena=False,
           batch=2, **extra):
    nd = dict(zip(("x", "w1", "w2", "w3", "wd"), needs))
    nd["wd"] = bool(down and nd["wd"])
    return dict(src="sweep", name=name, kind="bottleneck",
                inputs=dict(x=[batch, cin, 10, 14], w1=[p1, cin, 1, 1], w2=[p2, p1, 3, 3], w3=[cout, p2, 1, 1],
                            wd=[cout, cin, 1, 1] if down else None, in_relu=in_relu, out_premasked=premasked, stride=stride, needs=nd,
                            switches=sw or {}, arena=arena, fused=[False] * 4), **extra)


DEFECT_COUT66 = "Cout % 4 != 0: the forward rule lacks the term, so the data gradient goes to a Winograd entry that refuses 66 channels"


def sweep_rows():
    rows = []
    B2, B1 = (2, 10, 14), (1, 10, 14)        # 280 / 140 pixels: either side of the 224 cut; partial 4x4 tiles both ways
    x = lambda c, b=B2: (b[0], c, b[1], b[2])
    for cin in (60, 64, 66, 68):
        for cout in (60, 64, 66, 68):
            extra = dict(defect=DEFECT_COUT66) if (cin % 4 == 0 and cin >= 64 and cout == 66) else {}
            rows.append(_conv("c3_%d_%d" % (cin, cout), x(cin), (cout, cin, 3, 3), **extra))
    off = dict(train=dict(WINOGRAD_TRAIN=False), wgrad=dict(WINOGRAD_WGRAD=False), keepv=dict(WINOGRAD_KEEP_V=False),
               minc=dict(WINOGRAD_TRAIN_MIN_C=128))
    for key, sw in off.items():
        for allowed in (True, False):
            rows.append(_conv("c3_64_68_%s_off_%s" % (key, "wino" if allowed else "nowino"), x(64), (68, 64, 3, 3), winograd=allowed, sw=sw))
    for needs in ((True, True), (True, False), (False, True), (False, False)):
        for allowed in (True, False):
            rows.append(_conv("c3_64_68_needs%d%d_%s" % (needs + ("wino" if allowed else "nowino",)), x(64), (68, 64, 3, 3),
                              winograd=allowed, needs=needs))
    rows.append(_conv("c3_rpn", x(64), (68, 64, 3, 3), scale=False, winograd=False))          # bias + ReLU, forward kept direct
    rows.append(_conv("c3_64_68_res", x(64), (68, 64, 3, 3), res=True))
    rows.append(_conv("c3_64_68_s2", x(64), (68, 64, 3, 3), stride=2))
    rows.append(_conv("c3_64_68_pad0", x(64), (68, 64, 3, 3), pad=0))
    for b, tag in ((B1, "b1"), (B2, "b2")):
        for allowed in (True, False):
            rows.append(_conv("c3_64_68_arena_%s_%s" % (tag, "wino" if allowed else "nowino"), x(64, b), (68, 64, 3, 3), winograd=allowed, arena=True))
        rows.append(_conv("c1_64_68_arena_%s" % tag, x(64, b), (68, 64, 1, 1), pad=0, arena=True))
        rows.append(_conv("c1_64_68_%s" % tag, x(64, b), (68, 64, 1, 1), pad=0))
    for px, hw in ((224, (14, 16)), (225, (15, 15))):
        rows.append(_conv("c1_px%d_arena" % px, (1, 64, hw[0], hw[1]), (68, 64, 1, 1), pad=0, arena=True))
    n = 68 * 64 * 4
    for arena in (True, False):
        rows.append(_conv("c1_gw_fits_%d" % arena, x(64), (68, 64, 1, 1), pad=0, arena=arena, sw=dict(SMALL_GW_BYTES=n)))
        rows.append(_conv("c1_gw_over_%d" % arena, x(64), (68, 64, 1, 1), pad=0, arena=arena, sw=dict(SMALL_GW_BYTES=n - 4)))
    rows.append(_conv("c1_out", x(64), (68, 64, 1, 1), pad=0, res=True, out=True, needs=(False, False)))
    rows.append(_conv("c_whole_filter", (2, 16, 4, 4), (32, 16, 4, 4), scale=False, pad=0, winograd=False))
    rows.append(_conv("c_whole_filter_res", (2, 16, 4, 4), (32, 16, 4, 4), scale=False, pad=0, winograd=False, res=True))
    rows.append(_conv("c_whole_filter_1x1", (2, 16, 1, 1), (32, 16, 1, 1), scale=False, pad=0, winograd=False))
    rows.append(_conv("c1_fused", x(64), (68, 64, 1, 1), pad=0, fused=True))
    for m in (8, 96):                       # rows <= features, rows > features
        for nout in (64, 66):
            rows.append(_linear("l_%dx64_%d" % (m, nout), m, 64, nout))
            rows.append(_linear("l_%dx64_%d_floor" % (m, nout), m, 64, nout, sw=dict(LINEAR_DGRAD_AS_WGRAD=10 ** 9)))
    rows.append(_linear("l_96x64_65", 96, 64, 65))          # 3 zero filters
    rows.append(_linear("l_96x64_67", 96, 64, 67))
    rows.append(_linear("l_8x64_64_relu_nobias", 8, 64, 64, bias=False, relu=True))
    rows.append(_linear("l_8x64_64_x_only", 8, 64, 64, needs=(True, False)))
    rows.append(_linear("l_8x64_64_w_only", 8, 64, 64, needs=(False, True)))
    rows.append(_linear("l_8x64_64_arena", 8, 64, 64, arena=True))
    rows.append(_linear("l_96x64_64_arena", 96, 64, 64, arena=True))
    rows.append(_linear("l_8x64_64_fused", 8, 64, 64, fused=True))
    for p1, p2 in ((64, 64), (64, 60), (60, 64), (60, 66), (64, 66), (64, 68), (68, 64)):
        extra = dict(defect=DEFECT_COUT66) if (p1, p2) == (64, 66) else {}
        rows.append(_block("b_%d_%d" % (p1, p2), 256, p1, p2, 256, **extra))
    for key, sw in off.items():
        rows.append(_block("b_64_68_%s_off" % key, 256, 64, 68, 256, sw=sw))
    rows.append(_block("b_64_68_down_s2", 128, 64, 68, 256, down=True, stride=2))
    rows.append(_block("b_64_68_down", 128, 64, 68, 256, down=True, in_relu=True, premasked=True))
    rows.append(_block("b_64_68_w2_frozen", 256, 64, 68, 256, needs=(True, True, False, True, True)))
    rows.append(_block("b_64_68_x_frozen", 256, 64, 68, 256, needs=(False, True, True, True, True)))
    rows.append(_block("b_64_68_arena_b2", 256, 64, 68, 256, arena=True))
    rows.append(_block("b_64_68_arena_b1", 256, 64, 68, 256, arena=True, batch=1))
    raw = lambda name, kind, **inputs: dict(src="sweep", name=name, kind=kind, inputs=dict(inputs, switches={}))
    for m, nout in ((8, 64), (96, 64), (96, 66), (8, 66)):
        rows.append(raw("dgrad_raw_%d_%d" % (m, nout), "dgrad_raw", g=[m, nout, 1, 1], w=[nout, 64, 1, 1], x=[m, 64, 1, 1], stride=1, pad=0, arena=False))
    rows.append(raw("dgrad_raw_3x3_66", "dgrad_raw", g=[2, 66, 10, 14], w=[66, 64, 3, 3], x=[2, 64, 10, 14], stride=1, pad=1, arena=False))
    for arena in (False, True):
        rows.append(raw("wgrad_raw_1x1_%d" % arena, "wgrad_raw", x=[2, 64, 10, 14], g=[2, 68, 10, 14], w=[68, 64, 1, 1], stride=1, pad=0, arena=arena))
        rows.append(raw("wgrad_raw_3x3_%d" % arena, "wgrad_raw", x=[2, 64, 10, 14], g=[2, 68, 10, 14], w=[68, 64, 3, 3], stride=1, pad=1, arena=arena))
    return rows


def build_table(rows):
    out = []
    seen = set()
    for row in rows:
        key = json.dumps([row["kind"], row["inputs"]], sort_keys=True)
        if key in seen:
            continue
        seen.add(key)
        calls = trace(row["kind"], row["inputs"])
        route, place = derive_route(row["kind"], row["inputs"], calls)
        keep = {k: row[k] for k in ("src", "name", "kind", "inputs", "defect") if k in row}
        out.append(dict(keep, route=route, placement=place, calls=calls))
    return dict(note="written by tests/conv_trace.py on the commit before i2vsgg_amd/conv_route.py existed", rows=out)


def _dump(table):
    lines = ["  " + json.dumps(r, sort_keys=True) for r in table["rows"]]
    return '{"note": %s, "rows": [\n%s\n]}\n' % (json.dumps(table["note"]), ",\n".join(lines))


if __name__ == "__main__":
    recorded = []
    for path in sys.argv[1:]:
        with open(path) as f:
            data = json.load(f)
        recorded += data["rows"] if isinstance(data, dict) else data
    sys.stdout.write(_dump(build_table(recorded + sweep_rows())))
