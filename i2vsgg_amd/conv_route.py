"""Which kernel family serves a convolution layer's forward, data gradient and filter gradient: decided once per layer, here.

Pure host arithmetic on shapes and switches: no torch, no library, no state.  ``ops`` snapshots its switch attributes into a
``Switches`` record at each call, asks ``plan_conv`` once per layer and executes the ``Route`` it gets; the launch of each GEMM
inside a kernel family (tile, split, finish) is csrc/conv_plan.h's business.  tests/golden/conv_routes.json pins every route
below against the call traces of the code this module replaced ("Kernel routes of a conv layer")."""
from collections import namedtuple

EPI_RELU, EPI_RESIDUAL, EPI_SCALE, EPI_BIAS = 1, 2, 4, 8          # include/i2vsgg_hip.h (_lib mirrors them too)

DIRECT = "direct"                # the implicit-GEMM kernels (i2v_conv_fwd / _dgrad / _wgrad)
WINOGRAD = "winograd"            # F(4x4,3x3), the filter transformed per call: forward and data gradient
AS_WGRAD = "as_wgrad"            # a linear layer's data gradient as a filter gradient over the transposed output gradient
WINOGRAD_X = "winograd_x"        # filter gradient in the Winograd domain, the input transformed again
WINOGRAD_V = "winograd_v"        # ... from the transformed input the forward kept
NONE = "none"                    # nobody needs this gradient
ARENA, FRESH = "arena", "fresh"

Switches = namedtuple("Switches", "winograd_train winograd_wgrad winograd_keep_v winograd_train_min_c linear_dgrad_as_wgrad "
                                  "small_gw_bytes")
# fwd: DIRECT | WINOGRAD; keep_v: the Winograd forward also writes its transformed input; dgrad: NONE | DIRECT | WINOGRAD |
# AS_WGRAD; dgrad_pad: zero filters the direct data gradient appends (it reduces over Cout in float4s); transposed_g: the
# backward's epilogue pass also writes the output gradient transposed (for AS_WGRAD); wgrad: NONE | DIRECT | WINOGRAD_X |
# WINOGRAD_V; flags: the forward's EPI_* word; as_linear: the filter covers the whole input, the layer runs as a linear layer
# over the NHWC-flattened map (the other fields then describe that linear layer)
Route = namedtuple("Route", "fwd keep_v dgrad dgrad_pad transposed_g wgrad flags as_linear")


def whole_filter_as_linear(in_shape, w_shape, pad, has_res):
    """vrd.conv_lo's 8x8 layer: one output pixel.  As a conv its data gradient is a full correlation with 63 of 64 taps masked."""
    _, _, H, W = in_shape
    _, _, KH, KW = w_shape
    return pad == 0 and KH == H and KW == W and (KH > 1 or KW > 1) and not has_res


def epilogue_flags(scale, shift, res, relu):
    return (EPI_SCALE if scale else EPI_BIAS if shift else 0) | (EPI_RESIDUAL if res else 0) | (EPI_RELU if relu else 0)


def plan_dgrad(in_shape, w_shape, stride, pad, sw):
    """(AS_WGRAD | DIRECT, dgrad_pad) of a data gradient on the implicit-GEMM kernels: a layer's whose plan has not chosen
    Winograd, or one that is no layer of its own (netD_style's projections).
    A linear layer's gx[m][k] = sum_n g[m][n] w[n][k] is a 'filter gradient' whose pixel axis is n, whose activations are w as
    stored (n x k) and whose output gradient is g^T (n x m): only the small g is transposed, where the implicit-GEMM form
    re-lays the whole filter out first (fc7: 134 -> 48 us in the step, the 64-row layers 14-20 -> 10 us; Cout % 4 != 0: no
    zero-padded copies).  Only while g is the smaller of the two (rows <= in-features): netD_style's 37500-row projections keep
    the implicit-GEMM form, which reduces over Cout in float4s and so pads it with zero filters."""
    B, Cin, H, W = in_shape
    Cout, _, KH, KW = w_shape
    if ((H, W, KH, KW, stride, pad) == (1, 1, 1, 1, 1, 0) and B <= Cin
            and (Cout * Cin >= sw.linear_dgrad_as_wgrad or Cout % 4 != 0)):
        return AS_WGRAD, 0
    return DIRECT, (-Cout) % 4


def plan_conv(in_shape, w_shape, stride, pad, sw, scale=False, shift=False, res=False, relu=False, winograd_ok=False,
              needs_x=False, needs_w=False, needs_bias=False, in_block=False):
    """The route of one layer.  ``in_shape`` (B,Cin,H,W) and ``w_shape`` (Cout,Cin,KH,KW) are logical shapes; ``scale`` /
    ``shift`` / ``res`` / ``relu``: which epilogue operands exist; ``winograd_ok``: the caller allows a Winograd FORWARD (not the
    RPN's 3x3: proposal ranking between near-tied scores follows the conv's last bits, and the direct kernel's 1e-6 keeps 99 % of
    the reference's proposals, 1e-5 97 %); ``needs_*``: autograd's needs_input_grad (``needs_bias``: of a shift without scale);
    ``in_block``: conv2 of a bottleneck that is one autograd node (``ops.bottleneck``)."""
    as_linear = whole_filter_as_linear(in_shape, w_shape, pad, res)
    if as_linear:
        (B, Cin, H, W), Cout = in_shape, w_shape[0]
        in_shape, w_shape = (B, H * W * Cin, 1, 1), (Cout, H * W * Cin, 1, 1)
    B, Cin, H, W = in_shape
    Cout, _, KH, KW = w_shape
    flags = epilogue_flags(scale, shift, res, relu)
    # a trained stride-1 / pad-1 3x3 layer wide enough for the plane GEMMs to pay: forward and data gradient as F(4x4,3x3)
    eligible = (sw.winograd_train and (KH, KW, stride, pad) == (3, 3, 1, 1) and Cin >= sw.winograd_train_min_c
                and Cout >= sw.winograd_train_min_c and Cin % 4 == 0)
    # ... and its filter gradient, whose kernel also wants Cout in float4s
    wgrad_ok = eligible and sw.winograd_wgrad and Cout % 4 == 0
    if in_block:
        # As found, the block's rule tests no needs: the node exists because its filters train, its data gradient always runs
        # (conv1's filter gradient reads it) and follows the forward, and V is kept even when w2 itself is frozen.  It does not
        # ask ``winograd_ok`` either: a fused block ignores layers.WINOGRAD (known defect 2).  The fused data-gradient
        # entry is handed Cout as it is (no zero filters).
        fwd = WINOGRAD if eligible else DIRECT
        keep_v = bool(eligible and sw.winograd_keep_v and wgrad_ok)
        wgrad = NONE if not needs_w else (WINOGRAD_V if keep_v else WINOGRAD_X) if wgrad_ok else DIRECT
        return Route(fwd, keep_v, fwd, 0, False, wgrad, flags, as_linear)
    fwd_wino = bool(winograd_ok and eligible and (needs_x or needs_w) and not res)
    keep_v = bool(fwd_wino and sw.winograd_keep_v and needs_w and wgrad_ok)
    # The data gradient of an eligible 3x3 layer takes the Winograd form even where the forward may not (the RPN conv, a layer
    # with a residual operand): there it follows the filter gradient's rule.
    # KNOWN DEFECT 1, kept as found: the forward's rule lacks the ``Cout % 4`` term, so at Cout = 66 (Cin = 64, Winograd
    # allowed) the data gradient follows the forward to i2v_conv3x3_winograd4_fwd with 66 INPUT channels, which the library
    # refuses, while the filter gradient is direct.  No layer of the networks has such a channel count.
    dgrad_wino = fwd_wino or wgrad_ok
    plain, plain_pad = plan_dgrad(in_shape, w_shape, stride, pad, sw)
    dgrad = NONE if not needs_x else WINOGRAD if dgrad_wino else plain
    # the backward makes its one pass over the output gradient only for a ReLU mask, a BN scale or a bias sum; without that
    # pass the data-gradient wrapper transposes g itself
    transposed_g = bool(dgrad == AS_WGRAD and (relu or scale or needs_bias))
    # every eligible 3x3, the RPN's too: its FORWARD stays direct, the filter gradient only feeds the next step's weights
    wgrad = NONE if not needs_w else (WINOGRAD_V if keep_v else WINOGRAD_X) if wgrad_ok else DIRECT
    return Route(WINOGRAD if fwd_wino else DIRECT, keep_v, dgrad, plain_pad if dgrad == DIRECT else 0, transposed_g, wgrad,
                 flags, as_linear)


def wgrad_placement(n_elems, pixels, has_arena, sw):
    """Where a filter gradient of ``n_elems`` floats reduced over ``pixels`` output pixels goes: ARENA (the step's pre-zeroed
    arena, accumulated into with beta = 1: small filters split the pixel reduction over workgroups and add with atomics, one
    clear per step instead of one per call) or FRESH (its own tensor, beta = 0).  Up to 224 pixels the launcher never splits the
    reduction (fewer than 8 stages of 32): one workgroup per tile stores its result, no zeroed output needed."""
    return ARENA if has_arena and n_elems * 4 <= sw.small_gw_bytes and pixels > 224 else FRESH
