"""The kernel routes on the real library: for one row of tests/golden/conv_routes.json per distinct route combination, the layer's
forward and backward run with the recording proxy in pass-through mode.  The traced calls equal the row's (the wiring: what the
CPU trace of tests/test_conv_route_host.py records is what reaches the library), and y, gx and gw equal a float64 CPU reference
within the bounds tests/test_gpu_kernels.py holds the direct kernels and the Winograd path to.  B = 2 at 10x14: partial 4x4
tiles both ways and 280 pixels, above the 224-pixel cut of the arena placement; B = 1 for the side under it.  The rows with
an arena run inside an entered LaunchContext (beta = 1 into the pre-zeroed arena).  The Cout = 66 rows stay out: the library
refuses them (known defect 1).  The bottleneck rows check the calls and the output; the block's gradients against
torch, ReLU knife edges and all, are test_trained_bottleneck_stack_as_fused_autograd_nodes' in test_gpu_kernels.py."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_trace
from test_gpu_kernels import DEV, DIRECT_TOL, WINOGRAD_REL

pytestmark = pytest.mark.gpu

ROWS = ["c1_64_68_b2", "c3_64_68", "c3_rpn", "c3_64_68_keepv_off_wino", "c3_64_68_wgrad_off_wino", "c3_64_68_res", "c3_64_68_s2",
        "l_8x64_64", "l_96x64_64", "l_96x64_66", "l_8x64_64_x_only", "l_8x64_64_w_only", "c_whole_filter",
        "c1_64_68_arena_b2", "c1_64_68_arena_b1", "c3_64_68_arena_b2_wino", "l_96x64_64_arena", "b_64_68", "b_64_60", "b_64_68_arena_b2"]


@pytest.fixture(scope="module")
def table():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    with open(conv_trace.TABLE) as f:
        return {r["name"]: r for r in json.load(f)["rows"] if "name" in r}


def test_the_rows_cover_every_route_value(table):
    routes = [table[n]["route"] for n in ROWS]
    every = [r["route"] for r in table.values() if r["route"] is not None]
    for field in ("fwd", "keep_v", "dgrad", "transposed_g", "wgrad", "as_linear"):
        assert {r[field] for r in routes} == {r[field] for r in every}, field
    assert {table[n]["placement"] for n in ROWS} == {None, "arena", "fresh"}
    assert {tuple(table[n]["inputs"]["x"][:1] + table[n]["inputs"]["x"][2:]) for n in ROWS if n.startswith("c3")} == {(2, 10, 14)}
    assert not any("defect" in table[n] for n in ROWS)


def close(got, ref, winograd, what):
    got, ref = got.double().cpu(), ref.detach()
    if winograd:
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < WINOGRAD_REL, (what, err)
    else:
        np.testing.assert_allclose(got.numpy(), ref.numpy(), err_msg=what, **DIRECT_TOL)


def reference(kind, i, t):
    """y and the gradients in float64 on the CPU; the ReLU mask of the backward is the kernel's own (an output within 1e-5 of
    zero may sit on the other side in fp32)."""
    d = lambda k: t[k].detach().double().cpu().requires_grad_() if t.get(k) is not None else None
    x, w, shift, res = d("x"), d("w"), d("shift"), d("res")
    if kind == "linear":
        pre = F.linear(x, w, shift)
    else:
        pre = F.conv2d(x, w, None, i["stride"], i["pad"])
        if t.get("scale") is not None:
            pre = pre * t["scale"].double().cpu().view(1, -1, 1, 1)
        if shift is not None:
            pre = pre + shift.view(1, -1, 1, 1)
        if res is not None:
            pre = pre + res
    y = torch.relu(pre) if i["relu"] else pre
    if "gy" in t:
        mask = (t["y"] > 0).cpu() if i["relu"] else torch.ones_like(pre, dtype=torch.bool)
        (pre * mask * t["gy"].double().cpu()).sum().backward()
    return dict(y=y, gx=x.grad, gw=w.grad, gshift=shift.grad if shift is not None else None, gres=res.grad if res is not None else None)


def block_forward(i, t):
    d = lambda v: v.detach().double().cpu()
    bn = lambda h, k: h * d(t["bn"][k][0]).view(1, -1, 1, 1) + d(t["bn"][k][1]).view(1, -1, 1, 1)
    x = d(t["x"])
    a1 = torch.relu(bn(F.conv2d(x, d(t["w1"]), None, i["stride"]), "w1"))
    a2 = torch.relu(bn(F.conv2d(a1, d(t["w2"]), None, 1, 1), "w2"))
    skip = bn(F.conv2d(x, d(t["wd"]), None, i["stride"]), "wd") if t["wd"] is not None else x
    return torch.relu(bn(F.conv2d(a2, d(t["w3"])), "w3") + skip)


@pytest.mark.parametrize("name", ROWS)
def test_route_on_the_library(table, name):
    from i2vsgg_amd import launch
    row = table[name]
    kind, i, route = row["kind"], row["inputs"], row["route"]

    def run():
        with conv_trace.tracing(passthrough=True) as proxy:
            return proxy, conv_trace.run_layer(kind, i, proxy, device=DEV, seed=len(name))
    if i["arena"]:
        ctx = launch.LaunchContext(DEV)
        with ctx:                   # an eager pass sizes the arena, as a step's first one does
            run()
        ctx.fit()
        with ctx:
            proxy, t = run()
    else:
        proxy, t = run()
    torch.cuda.synchronize()
    assert proxy.calls == row["calls"]
    if kind == "bottleneck":
        close(t["y"], block_forward(i, t), route["fwd"] == "winograd", "y")
        assert all(t["g" + k] is not None and bool(torch.isfinite(t["g" + k]).all()) for k in ("x", "w1", "w2", "w3"))
        return
    ref = reference(kind, i, t)
    wino = dict(y=route["fwd"] == "winograd", gx=route["dgrad"] == "winograd", gw=route["wgrad"].startswith("winograd"),
                gshift=False, gres=False)
    need = i["needs"]
    for k, needed in (("y", True), ("gx", need["x"]), ("gw", need["w"]), ("gshift", need.get("shift")), ("gres", need.get("res"))):
        assert (t.get(k) is not None) == bool(needed), k
        if needed:
            close(t[k].reshape(ref[k].shape), ref[k], wino[k], k)
