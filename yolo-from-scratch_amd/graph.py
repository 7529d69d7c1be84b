"""Static network plans over NHWC buffers: the host-side scheduler of the HIP kernels.

A module tree is *traced once* per (input shape, mode) into a list of layer records over symbolic
NHWC buffers; the records are lowered to two flat op lists (forward, backward) of `yh_op` structs
holding raw device pointers.  Running a step is then two C calls (`yh_run`) -- no per-layer Python,
no autograd graph, no allocation -- which is what makes the lists hipGraph-friendly.

Design points (all about HBM traffic, the bound for this small-channel network):
  * torch.cat never materialises: producers write straight into channel slices of a shared buffer
    (a view = buffer + channel offset, ld = buffer channels);
  * nearest-x2 upsampling is folded into the producer's BN+SiLU write, the residual add into the
    same pass; the head outputs are already (B,G,G,3,5+nc) because the layout is NHWC;
  * BatchNorm statistics come out of the conv epilogue; dY overwrites Y in place in the backward.
"""
from __future__ import annotations

import ctypes
import os
import struct
from collections import defaultdict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L

BN_EPS_DEFAULT = 1e-5
# bumped whenever this package's kernels modify parameters or BatchNorm buffers in place (see Plan.weights_state)
WEIGHTS_EPOCH = [0]
# bumped whenever this package moves parameter / buffer STORAGE (HipTrainer adopting the parameters into its flat buffer,
# Module._apply: .to() / .cuda() / .float(), load_state_dict): plans and captured hipGraphs hold raw addresses
PARAM_GENERATION = [0]


def _on_reregistration(module, name, value):
    """Global torch hook: a parameter or buffer attribute that already held a tensor is being REPLACED (`conv.weight =
    nn.Parameter(...)`, `bn.running_mean = t`, load_state_dict(assign=True) through any parent module).  Plans and captured
    hipGraphs hold the old tensor's address: bump the generation so every holder re-validates (the per-image check of
    InferenceSession compares this counter instead of walking the module tree)."""
    for store in ("_parameters", "_buffers"):
        d = module.__dict__.get(store)
        if d is not None and d.get(name) is not None and d.get(name) is not value:
            PARAM_GENERATION[0] += 1
            return None
    return None


torch.nn.modules.module.register_module_parameter_registration_hook(_on_reregistration)
torch.nn.modules.module.register_module_buffer_registration_hook(_on_reregistration)


def invalidate_folded_weights():
    """Tell every eval plan / InferenceSession that parameter or BatchNorm-buffer VALUES changed behind torch's version
    counters.  The package calls this itself wherever its own code writes parameter storage (optimizer kernels, training
    forwards, HipTrainer's broadcast, load_state_dict); user code must call it after writes torch cannot see on the
    registered tensors: `p.data.mul_()` / `p.data.copy_()` (`.data` carries its own version counter -- the usual EMA idiom),
    writes through an aliasing view such as `trainer.flat_p`, and in-place collectives on parameters."""
    WEIGHTS_EPOCH[0] += 1


def state_token():
    """One cheap comparison for 'nothing this package knows of has touched the weights or their addresses'."""
    return (WEIGHTS_EPOCH[0], PARAM_GENERATION[0])


def _rup4(c: int) -> int:
    return (c + 3) // 4 * 4


def _rup8(c: int) -> int:
    return (c + 7) // 8 * 8


# op kinds of the passes whose fp32 and bf16 forms take the same arguments
_OPS = {False: dict(pool=L.OP_MAXPOOL5_FWD, pool_bwd=L.OP_MAXPOOL5_BWD, reduce=L.OP_BN_SILU_BWD_REDUCE, apply=L.OP_BN_SILU_BWD_APPLY,
                    colsum=L.OP_COLSUM, wgrad=L.OP_CONV_BWD_WEIGHT, narrow_w=L.OP_CONV_NARROW_BWD_WEIGHT, narrow=L.OP_CONV_NARROW,
                    narrow_s2=L.OP_CONV_NARROW_DGRAD_S2, dgrad=L.OP_CONV_BWD_DATA),
        True: dict(pool=L.OP_BF16_MAXPOOL5_FWD, pool_bwd=L.OP_BF16_MAXPOOL5_BWD, reduce=L.OP_BF16_BN_SILU_BWD_REDUCE,
                   apply=L.OP_BF16_BN_SILU_BWD_APPLY, colsum=L.OP_BF16_COLSUM, wgrad=L.OP_BF16_CONV_BWD_WEIGHT,
                   narrow_w=L.OP_BF16_CONV_NARROW_BWD_WEIGHT, narrow=L.OP_BF16_CONV_NARROW, narrow_s2=L.OP_BF16_CONV_NARROW_DGRAD_S2,
                   dgrad=L.OP_BF16_CONV_BWD_DATA)}
# weight-transform launches (*_MULTI: one descriptor per conv) in the order they run, with the descriptor layout of each
_TABLES = [(L.OP_FOLD_OIHW_MULTI, "<QQQQQQQQiifi"), (L.OP_PACK_WEIGHTS_MULTI, "<QQQiiiiiiii"), (L.OP_BF16_PACK_MULTI, "<QQQiiiiiiii"),
           (L.OP_WINO_WEIGHTS_MULTI, "<QQiiii"), (L.OP_LAT_PACK_MULTI, "<QQiiii"), (L.OP_PW_PACK_MULTI, "<QQQiiiiii")]


class Buffer:
    """An NHWC activation tensor (B,H,W,C) -- fp32, or bf16 on the bf16 path -- plus, lazily, its gradient tensor.
    The gradient may have its own type and pixel stride: the bf16 path's head outputs stay fp32 (they feed the fp32
    loss) while their gradient is bf16 with the channel axis zero-padded to a multiple of 8 (grad_C)."""

    def __init__(self, plan: "Plan", B: int, H: int, W: int, C: int, name: str, dtype: Optional[torch.dtype] = None,
                 grad_C: Optional[int] = None):
        self.plan, self.B, self.H, self.W, self.C, self.name = plan, B, H, W, C, name
        self.dtype = dtype if dtype is not None else plan.act_dtype
        self.grad_dtype, self.grad_C = plan.act_dtype, (grad_C if grad_C is not None else C)
        self.data = torch.empty(B, H, W, C, device=plan.device, dtype=self.dtype)
        self._grad: Optional[torch.Tensor] = None
        self.grad_cover: List[Tuple[int, int]] = []   # channel ranges already written in this backward
        self._icoef: Optional[torch.Tensor] = None

    @property
    def icoef(self) -> torch.Tensor:
        """Input-prologue table of the buffer's channels, rows [scale | shift | gate] (see yh_prologue in csrc/common.h): channels
        whose producer's BatchNorm + SiLU is applied by the READERS (the activation is never materialised, the buffer holds the raw
        convolution output) carry the producer's scale / shift (rewritten by its bn_finalize every step) and gate 1; all others
        the identity (1, 0, gate 0)."""
        if self._icoef is None:
            ld = _rup4(self.C) + 4
            t = torch.zeros(3, ld, device=self.plan.device, dtype=torch.float32)
            t[0].fill_(1.0)
            self._icoef = t
        return self._icoef

    @property
    def grad(self) -> torch.Tensor:
        if self._grad is None:      # zeros: padding channels of a padded gradient must stay finite (they meet zero weights)
            self._grad = torch.zeros(self.B, self.H, self.W, self.grad_C, device=self.plan.device, dtype=self.grad_dtype)
        return self._grad

    def view(self, off: int = 0, C: Optional[int] = None) -> "View":
        return View(self, off, self.C - off if C is None else C)


@dataclass
class View:
    buf: Buffer
    off: int
    C: int

    @property
    def B(self): return self.buf.B
    @property
    def H(self): return self.buf.H
    @property
    def W(self): return self.buf.W
    @property
    def ld(self): return self.buf.C
    @property
    def ldg(self): return self.buf.grad_C
    @property
    def M(self): return self.buf.B * self.buf.H * self.buf.W
    @property
    def aligned4(self) -> bool:
        """Row stride and channel offset are multiples of 4: the view is addressable in 4-channel pieces (16 bytes fp32)."""
        return self.buf.C % 4 == 0 and self.off % 4 == 0
    def ptr(self) -> int: return self.buf.data.data_ptr() + self.buf.data.element_size() * self.off
    def gptr(self) -> int: return self.buf.grad.data_ptr() + self.buf.grad.element_size() * self.off
    def icoef_ptr(self, row: int = 0) -> int: return self.buf.icoef.data_ptr() + 4 * (row * self.buf.icoef.shape[1] + self.off)
    @property
    def icoef_ld(self) -> int: return self.buf.icoef.shape[1]


def _same_view(a: "View", b: "View") -> bool:
    return a.buf is b.buf and a.off == b.off and a.C == b.C


@dataclass
class ConvRec:
    """conv (+bias) [+ BatchNorm + SiLU (+residual) (+x2 upsample on write)]"""
    x: View
    out: View
    weight: torch.nn.Parameter
    bias: Optional[torch.nn.Parameter]
    bn: Optional[torch.nn.BatchNorm2d]
    k: int
    s: int
    residual: Optional[View] = None
    upsample: bool = False
    # filled by the planner
    cin: int = 0            # padded input channels seen by the kernels
    cout: int = 0
    Ho: int = 0
    Wo: int = 0
    y: Optional[torch.Tensor] = None        # raw conv output (B,Ho,Wo,cout); dY overwrites it in the backward
    coef: Optional[torch.Tensor] = None
    part: Optional[torch.Tensor] = None
    wf: Optional[torch.Tensor] = None
    wb: Optional[torch.Tensor] = None
    ldwf: int = 0
    ldwb: int = 0
    need_dx: bool = True
    lane: int = 0
    wino_f: bool = False    # forward on the Winograd F(2x2,3x3) kernel
    wino_b: bool = False    # backward-data on the Winograd kernel
    wino_w: bool = False    # backward-weight in the Winograd domain
    pw_w: bool = False      # backward-weight on the pointwise (1x1) kernel
    pw_f: bool = False      # forward on the pointwise GEMM kernel
    s2m_b: bool = False     # stride-2 backward-data with the column parities merged into the channel axis
    narrow_f: bool = False  # forward on the direct kernel for the narrow high-resolution 3x3 layers
    narrow_b: bool = False  # stride-1 backward-data on the same kernel (flipped taps)
    narrow_w: bool = False  # weight gradient on the direct pixel-reduction kernel
    s2l_f: bool = False     # forward on the LDS-staged 3x3 stride-2 kernel (conv_s2.hip)
    cin_k: int = 0          # input channels the narrow kernels read (bf16 plan: 4 of the first layer's 8 padded ones)
    fwd2: bool = False      # forward fused with the sibling pointwise conv (one GEMM, N = cout1 + cout2)
    nblk: int = 0           # BatchNorm partial-sum rows written by the forward kernel
    pw_b: bool = False      # backward-data on the pointwise GEMM kernel
    pair: Optional["ConvRec"] = None       # sibling pointwise conv reading the same input (fused backward-data)
    pair_first: bool = False
    conv: Optional[torch.nn.Conv2d] = None  # the parameter container (staleness checks look the parameters up again)
    virtual: bool = False   # the activation is never materialised: the conv writes its raw output into `out`, readers apply BN + SiLU
    x_fused: bool = False   # the input view has virtual channels: forward / weight-gradient kernels run the input prologue
    yp: int = 0             # address and pixel stride of the raw conv output (private tensor `y`, or the `out` view when virtual)
    ldy: int = 0
    dyp: int = 0            # where the BatchNorm backward writes dY: over Y in place, or (virtual) into the private tensor `y` -- the
    lddy: int = 0           # raw output in the shared buffer is still being read by the consumers' weight gradients on the side lane
    kcout_b: int = 0        # K rows of the backward-data pack (> cout: a head whose gradient rows are zero-padded; 0: cout)
    eval_fam: str = ""      # eval plan: "wino" | "pw" | "lat" | "" (gather-GEMM) fused forward; the training flags stay False


@dataclass
class PoolRec:
    x: View
    out: View
    arg: Optional[torch.Tensor] = None
    lane: int = 0
    fused: bool = False     # eval: computed by the preceding pool's three-stage launch


@dataclass
class SyncRec:
    """fork (side lane may start) / join (main lane waits for the side lane) marker in the forward order"""
    kind: str


class Plan:
    """Trace target + compiled op lists for one module at one input shape / mode."""

    def __init__(self, device: torch.device, in_shape: Tuple[int, int, int, int], training: bool, need_input_grad: bool,
                 dtype: str = "f32"):
        if dtype not in ("f32", "bf16"):
            raise ValueError(f"compute dtype must be 'f32' or 'bf16', got {dtype!r}")
        if dtype == "bf16" and not training:
            raise NotImplementedError("the bf16 path covers training plans; eval plans run the fp32 fused kernels")
        self.device, self.training, self.need_input_grad = device, training, need_input_grad
        self.dtype = dtype
        self.bf16 = dtype == "bf16"
        self.act_dtype = torch.bfloat16 if self.bf16 else torch.float32
        self.B, self.Cimg, self.Himg, self.Wimg = in_shape
        self.recs: List[object] = []
        self.buffers: List[Buffer] = []
        self.outputs: List[Tuple[View, str]] = []       # (view, "nhwc_heads" | "nchw")
        self.input = self.new_buffer(self.B, self.Himg, self.Wimg, (_rup8 if self.bf16 else _rup4)(self.Cimg), "input")
        self.generation = 0
        self.lane = 0                      # lane given to records traced from now on (see side_lane())
        self.fwd_ops = self.bwd_ops = None
        self.param_ptrs: List[int] = []
        self._sig_holders = None
        self._grad_of = None
        self.prep_ops = None               # eval plans: BatchNorm folding, run once per weight state
        self._fold_tensors = None
        self._folded_state = None

    # ---- tracing API used by the modules ------------------------------------------------------
    def new_buffer(self, B, H, W, C, name="act", dtype=None, grad_C=None) -> Buffer:
        b = Buffer(self, B, H, W, C, name, dtype, grad_C)
        self.buffers.append(b)
        return b

    def conv(self, x: View, conv: torch.nn.Conv2d, bn: Optional[torch.nn.BatchNorm2d], out: Optional[View] = None,
             residual: Optional[View] = None, upsample: bool = False) -> View:
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        if conv.kernel_size[0] != conv.kernel_size[1] or k not in (1, 3) or s not in (1, 2) or p != k // 2 \
                or conv.stride[0] != conv.stride[1] or conv.groups != 1 or conv.dilation != (1, 1):
            raise NotImplementedError(f"HIP conv path supports square k in (1,3), stride in (1,2), padding k//2; got {conv}")
        if (k, s) == (1, 2):
            raise NotImplementedError("1x1 stride-2 convolutions are not part of this network")
        if conv.in_channels != x.C and (_rup8 if self.bf16 else _rup4)(conv.in_channels) != x.C:
            raise ValueError(f"conv expects {conv.in_channels} input channels, got a view with {x.C}")
        if self.bf16 and (x.C % 8 or x.ld % 8 or x.off % 8 or (bn is not None and conv.out_channels % 8)):
            raise NotImplementedError("the bf16 path needs channel counts, views and strides in multiples of 8")
        Ho, Wo = (x.H + 2 * p - k) // s + 1, (x.W + 2 * p - k) // s + 1
        cout = conv.out_channels
        if bn is not None and cout % 4:
            raise NotImplementedError("Conv+BN+SiLU on the HIP path needs out_channels % 4 == 0")
        f = 2 if upsample else 1
        if out is None and self.bf16 and bn is None:
            # a plain conv output on the bf16 path (the detection heads): fp32 values for the fp32 loss, bf16 gradient
            # with the channel axis zero-padded to a multiple of 8 (the backward GEMMs read 16-byte pieces)
            out = self.new_buffer(x.B, Ho * f, Wo * f, cout, "head", dtype=torch.float32, grad_C=_rup8(cout)).view()
        if out is None and bn is None:
            # a plain conv output (the detection heads, 3 (5 + nc) = 18 / 255 channels): dense values for the loss, but a gradient whose
            # pixel rows are zero-padded to a multiple of 4 channels -- the backward GEMMs and the bias column sum then read 16-byte
            # pieces (at nc = 80 the 255-float rows ran every one of them on its scalar-load variant)
            out = self.new_buffer(x.B, Ho * f, Wo * f, cout, "head", grad_C=_rup4(cout)).view()
        if out is None:
            out = self.new_buffer(x.B, Ho * f, Wo * f, _rup4(cout)).view()
        if self.bf16 and bn is not None and (out.off % 8 or out.ld % 8):
            raise NotImplementedError("the bf16 path needs output views aligned to 8 channels")
        if self.bf16 and bn is None and out.buf.dtype != torch.float32:
            raise NotImplementedError("plain conv outputs on the bf16 path are fp32 head tensors")
        if (out.H, out.W, out.C) != (Ho * f, Wo * f, cout):
            raise ValueError(f"output view {(out.H, out.W, out.C)} does not match conv result {(Ho * f, Wo * f, cout)}")
        if residual is not None and (residual.H, residual.W, residual.C) != (Ho, Wo, cout):
            raise ValueError("residual shape mismatch")
        self.recs.append(ConvRec(x, out, conv.weight, conv.bias, bn, k, s, residual, upsample, cin=x.C, cout=cout,
                                 Ho=Ho, Wo=Wo, lane=self.lane, conv=conv))
        return out

    # independent sub-graphs: `with plan.side_lane():` traces the enclosed layers onto the side stream;
    # a fork marker is emitted on entry (the side lane sees everything traced before), the join is emitted
    # by `join()` (or implicitly at the end of the op list)
    def side_lane(self):
        plan = self

        enabled = True

        class _Ctx:
            def __enter__(self_inner):
                if enabled:
                    plan.recs.append(SyncRec("fork"))
                    plan.lane = 1

            def __exit__(self_inner, *exc):
                plan.lane = 0
        return _Ctx()

    def join(self):
        self.recs.append(SyncRec("join"))

    def pool5(self, x: View, out: View) -> View:
        if x.C % 4 or (x.H, x.W, x.C) != (out.H, out.W, out.C):
            raise ValueError("pool5: shape mismatch or channels not a multiple of 4")
        self.recs.append(PoolRec(x, out, lane=self.lane))
        return out

    def mark_output(self, v: View, kind: str):
        self.outputs.append((v, kind))

    # ---- lowering -----------------------------------------------------------------------------
    def params(self) -> List[torch.nn.Parameter]:
        seen, out = set(), []
        for r in self.recs:
            if isinstance(r, ConvRec):
                for p in (r.weight, r.bias, r.bn.weight if r.bn is not None else None,
                          r.bn.bias if r.bn is not None else None):
                    if p is not None and id(p) not in seen:
                        seen.add(id(p))
                        out.append(p)
        return out

    # ---- kernel-family routing: decided for every record before anything is lowered ------------------------------------------
    # A family is admitted by plan-level conditions plus the library's own query (`*_ok`, `*_blocks`); a launcher condition that no
    # query reports is written here next to a reference to the launcher.
    def _convs(self) -> List[ConvRec]:
        return [r for r in self.recs if isinstance(r, ConvRec)]

    def _pair_siblings(self, mult: int) -> List[ConvRec]:
        """Sibling pointwise convs reading the same input (C3 conv1 / conv2) share one backward-data GEMM over K = Cout1 + Cout2,
        dx written once.  `mult`: the channel multiple the pair's GEMM needs.  Returns the first of each pair."""
        groups: Dict[tuple, List[ConvRec]] = {}
        for r in self._convs():
            if r.k == 1 and r.s == 1 and r.bn is not None and r.cout % mult == 0:
                groups.setdefault((id(r.x.buf), r.x.off, r.x.C), []).append(r)
        firsts = []
        for grp in groups.values():
            if len(grp) == 2 and grp[0].cout == grp[1].cout and (self.need_input_grad or grp[0].x.buf is not self.input):
                a, b = grp
                a.pair, b.pair, a.pair_first = b, a, True
                firsts.append(a)
        return firsts

    @staticmethod
    def _wino_shape(r: ConvRec) -> bool:
        return r.k == 3 and r.s == 1 and r.cin == r.weight.shape[1] and r.x.aligned4 and r.x.H % 2 == 0 and r.x.W % 2 == 0

    def _wino_lds_ok(self, r: ConvRec, K: int) -> bool:
        """Forward (K = Cin) or backward-data (K = Cout) on the LDS-staged Winograd kernel: launch_wino_lds needs K % 16 and a block
        geometry for (B, H, W)."""
        return self._wino_shape(r) and K % 16 == 0 and K <= 2048 and L.lib().yh_conv_wino_blocks(r.x.B, r.x.H, r.x.W) > 0

    @staticmethod
    def _pw_fits(M: int, ld: int, K: int) -> bool:
        return 4 * ((M - 1) * ld + K) < 1 << 31        # launch_pw_gemm (conv_pw.hip): 32-bit byte offsets into the input

    def _pw_ok(self, r: ConvRec) -> bool:
        """Pointwise GEMM forward: measured faster than the gather-GEMM except when both K and N are >= 256."""
        return r.k == 1 and r.s == 1 and r.cin == r.weight.shape[1] and r.x.aligned4 and r.cin % 8 == 0 and \
            not (r.cin >= 256 and r.cout >= 256) and self._pw_fits(r.x.M, r.x.ld, r.cin)

    def _route_f32(self, r: ConvRec, special: bool):
        """Which kernel family runs each pass of one convolution (fp32 training).  The fusion planner (_plan_fusion) needs it for
        every record: whether every reader of a tensor can apply the producer's BatchNorm + SiLU itself."""
        lib = L.lib()
        r.ldwb, r.ldwf, r.cin_k = _rup4(r.cin), _rup4(r.cout), r.cin
        r.need_dx = self.need_input_grad or r.x.buf is not self.input
        unpadded = r.cin == r.weight.shape[1]
        r.wino_f = special and self._wino_lds_ok(r, r.cin)
        r.wino_b = special and r.need_dx and self._wino_lds_ok(r, r.cout)
        r.wino_w = special and self._wino_shape(r) and r.cin % 32 == 0 and r.cout % 32 == 0 and r.x.W >= 4
        r.pw_w = special and r.k == 1 and r.s == 1 and unpadded
        r.pw_f = special and self._pw_ok(r)
        r.s2m_b = special and r.k == 3 and r.s == 2 and r.need_dx and r.cin <= 16 and r.x.ld == r.cin and r.x.W % 2 == 0 and unpadded
        # narrow high-resolution 3x3 layers: direct kernel (LDS halo patch, filter in registers, 16-wide MFMA tiles); the first
        # layer runs it with CIN = 4 (3 channels padded)
        nar = special and r.k == 3 and unpadded and r.x.aligned4
        r.narrow_f = bool(special and r.k == 3 and r.x.aligned4 and (unpadded or r.x.ld == r.cin == 4)
                          and lib.yh_conv_narrow_ok(r.cin, r.cout, 3, r.s))
        r.s2l_f = bool(special and not r.narrow_f and r.k == 3 and r.s == 2 and unpadded and r.x.aligned4 and
                       lib.yh_conv_s2_ok(r.x.B, r.x.H, r.x.W, r.cin, r.cout))
        r.narrow_b = bool(nar and r.s == 1 and r.need_dx and lib.yh_conv_narrow_ok(r.cout, r.cin, 3, 1))
        if r.narrow_f:
            r.wino_f = False
        if r.narrow_b:
            r.wino_b = False
        if nar and r.s == 2 and r.need_dx and lib.yh_conv_narrow_dgrad_s2_ok(r.cin, r.cout):
            r.narrow_b, r.s2m_b = True, False      # the stride-2 form of the direct backward-data kernel
        r.narrow_w = bool(special and r.k == 3 and r.x.aligned4 and lib.yh_conv_narrow_bwd_weight_ok(r.cin, r.weight.shape[1], r.cout, 3, r.s))
        if r.narrow_w:
            r.wino_w = False
        # backward-data on the pointwise GEMM: N = Cin, K = Cout (+ the sibling's Cout), dY rows of Cout (the first's) channels
        pw_in = special and r.k == 1 and r.s == 1 and unpadded and r.x.aligned4 and r.need_dx
        lddy = r.cout if r.bn is not None else r.out.ldg
        if r.pair is None:
            r.pw_b = pw_in and r.cout % 8 == 0 and not (r.cout >= 256 and r.cin >= 256) and self._pw_fits(r.x.M, lddy, r.cout)
        elif r.pair_first:
            kpair = r.cout + r.pair.cout
            r.pw_b = r.pair.pw_b = pw_in and r.cout % 8 == 0 and r.pair.cout % 8 == 0 and not (kpair >= 256 and r.cin >= 256) \
                and self._pw_fits(r.x.M, r.cout, kpair)

    def _route_bf16(self, r: ConvRec):
        """bf16 training: the bf16 gather-GEMM family (yh_bf16_conv_fwd / _bwd_data / _bwd_weight: bf16 operands, fp32 accumulation)
        for every pass, except the narrow direct kernels of the fp32 path with bf16 storage (conv_narrow.hip) where they measured
        faster.  cin_k = channels the narrow kernels read (4 of the first layer's 8 padded ones)."""
        lib = L.lib()
        cin_real = r.weight.shape[1]
        r.need_dx = self.need_input_grad or r.x.buf is not self.input
        r.ldwf, r.ldwb = _rup8(r.cout), _rup8(r.cin)
        r.cin_k = 4 if (cin_real <= 4 and r.cin == 8) else r.cin
        if r.bn is None:        # head: the loss writes a bf16 gradient zero-padded to a multiple of 8 channels
            r.kcout_b = _rup8(r.cout)
            if r.out.off != 0 or r.out.ldg != r.kcout_b:
                raise NotImplementedError("head gradient must own its (padded) buffer")
        # measured at batch 64 (tools/layer_bench.py --dtype bf16, ms narrow / generic bf16): first layer forward 0.250 / 0.358 and
        # weight gradient 0.220 / 0.541; stem[3] forward 0.250 / 0.114, backward-data 0.295 / 0.338, weight gradient 0.274 / 0.155;
        # 16 -> 16 forward 0.098 / 0.098, backward-data 0.114 / 0.099, weight gradient 0.113 / 0.129 per layer (8-byte pieces: twice
        # the load instructions per byte of the fp32 form -- these kernels are bound by instruction issue and latency, not by
        # bytes).  Each pass takes the faster kernel.  Round 3: stem[3] forward (16 -> 32, stride 2) has a bf16-MFMA form of the
        # narrow kernel (0.112 -> 0.075 ms).
        nar = r.k == 3 and r.bn is not None and r.x.aligned4
        stem3 = r.s == 2 and r.cin == 16 and r.cout == 32 and r.cin == cin_real
        r.narrow_f = bool(nar and (r.cin_k == 4 or stem3) and lib.yh_conv_narrow_ok(r.cin_k, r.cout, 3, r.s))
        r.narrow_w = bool(nar and (r.cin_k == 4 or r.s == 1) and
                          lib.yh_conv_narrow_bwd_weight_ok(r.cin_k, min(cin_real, r.cin_k), r.cout, 3, r.s))
        r.narrow_b = bool(nar and r.need_dx and r.pair is None and r.cin == cin_real and r.s == 2 and
                          lib.yh_conv_narrow_dgrad_s2_ok(r.cin, r.cout))

    def _route_eval(self, r: ConvRec):
        """Eval: one fused kernel per conv -- conv + folded-BN bias + SiLU (+residual) (+x2 upsample).  Winograd / pointwise GEMM for
        layers with enough workgroups to fill the chip (eval_epoch, predict_batch), the latency kernel (conv_lat.hip: K split over the
        waves of a workgroup, no split-K slabs / fences) for the small-M layers of batch-1 inference, the gather-GEMM with in-launch
        split-K otherwise.  Recorded in eval_fam; the training flags stay False."""
        r.ldwb, r.ldwf = _rup4(r.cin), _rup4(r.cout)
        fast = os.environ.get("YH_EVAL_FAST", "1") != "0"
        M = r.x.B * r.Ho * r.Wo
        # lat: measured at batch 1, 640x640, end to end / device ms with the uint8 image: off 1.283 / 1.227, M <= 8192 0.955 / 0.842,
        # M <= 32768 0.954 / 0.845, every layer 0.924 / 0.842 -- the 160x160 layers are a wash, larger M belongs to the throughput kernels
        if fast and self._wino_lds_ok(r, r.cin) and ((M // 4 + 31) // 32) * ((r.cout + 63) // 64) >= 192:
            r.eval_fam = "wino"
        elif fast and self._pw_ok(r) and ((M + 127) // 128) * ((r.cout + 127) // 128) >= 128:
            r.eval_fam = "pw"
        elif fast and M <= 32768 and r.cin == r.weight.shape[1] and r.x.aligned4 and \
                L.lib().yh_conv_lat_ok(r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s):
            r.eval_fam = "lat"

    def _plan_fusion(self, special: bool):
        """Decide which Conv+BN+SiLU outputs are never materialised ("virtual"): the convolution writes its RAW output straight
        into the output view (a channel slice of the consumer's buffer), bn_finalize publishes scale / shift in the buffer's
        prologue table, and every reader -- forward kernel, weight-gradient kernel, residual add -- applies scale, shift and SiLU
        while it stages its operand (train.py:253-265 executed at the consumer).  Saves the whole bn_silu_fwd round trip (8 bytes
        per element fp32).  A tensor stays materialised when it carries a residual or an upsample, is a plan output, feeds a
        max-pool, or has a reader whose kernel family has no prologue.  fp32 training plans only."""
        readers: Dict[int, List[tuple]] = {}
        for r in self.recs:
            if isinstance(r, ConvRec):
                readers.setdefault(id(r.x.buf), []).append((r.x.off, r.x.C, "conv", r))
                if r.residual is not None:
                    readers.setdefault(id(r.residual.buf), []).append((r.residual.off, r.residual.C, "res", r))
            elif isinstance(r, PoolRec):
                readers.setdefault(id(r.x.buf), []).append((r.x.off, r.x.C, "pool", r))
        outs = [(id(v.buf), v.off, v.C) for v, _ in self.outputs]
        enabled = special and os.environ.get("YH_FUSE_ACT", "1") != "0"

        def overlap(o1, c1, o2, c2):
            return o1 < o2 + c2 and o2 < o1 + c1
        for r in self.recs:
            if not isinstance(r, ConvRec) or r.bn is None:
                continue
            v = r.out
            ok = enabled and not r.upsample and r.residual is None and v.off % 4 == 0 and v.C % 4 == 0
            ok = ok and not any(b == id(v.buf) and overlap(v.off, v.C, o, c) for b, o, c in outs)
            n_read = 0
            for off, C, kind, c in readers.get(id(v.buf), []):
                if not ok or not overlap(v.off, v.C, off, C):
                    continue
                n_read += 1
                if kind == "pool":
                    ok = False
                elif kind == "conv":
                    ok = self._fwd_prologue_ok(c) and self._wgrad_prologue_ok(c)
            r.virtual = bool(ok and n_read > 0)
        for r in self.recs:                      # readers of virtual channels
            if isinstance(r, ConvRec):
                r.x_fused = any(isinstance(q, ConvRec) and q.virtual and q.out.buf is r.x.buf and overlap(q.out.off, q.out.C, r.x.off, r.x.C)
                                for q in self.recs)
        for r in self.recs:
            if isinstance(r, ConvRec) and r.virtual:
                r.out.buf.icoef[2, r.out.off: r.out.off + r.out.C] = 1.0

    def _fwd_prologue_ok(self, c: "ConvRec") -> bool:
        """Forward kernel families that can apply the producer's BatchNorm + SiLU while staging their input."""
        lib = L.lib()
        if not c.x.aligned4 or c.cin % 4 or c.cin != c.weight.shape[1]:
            return False
        M = c.x.B * c.Ho * c.Wo
        if c.narrow_f:
            return c.cin == 16
        if c.wino_f or c.s2l_f:
            return True
        if c.fwd2:
            return bool(lib.yh_conv_pw_prologue_ok(M, c.cin, c.cout + c.pair.cout))
        if c.pw_f:
            return bool(lib.yh_conv_pw_prologue_ok(M, c.cin, c.cout))
        return True                                   # gather-GEMM: 16-byte staging of 4-channel pieces

    def _wgrad_prologue_ok(self, c: "ConvRec") -> bool:
        lib = L.lib()
        if not c.x.aligned4 or c.cin % 4 or c.cin != c.weight.shape[1]:
            return False
        if c.narrow_w:
            return c.cin == 16
        if c.wino_w or c.pw_w:
            return True
        return bool(lib.yh_conv_bwd_weight_prologue_ok(c.x.B, c.x.H, c.x.W, c.cin, c.cout, c.k, c.s))

    def _res_fused(self, r: "ConvRec") -> bool:
        v = r.residual
        return v is not None and any(isinstance(q, ConvRec) and q.virtual and q.out.buf is v.buf and
                                     q.out.off < v.off + v.C and v.off < q.out.off + q.out.C for q in self.recs)

    # ---- lowering -----------------------------------------------------------------------------------------------------------
    def compile(self, grad_of: Optional[Dict[int, torch.Tensor]] = None):
        """Allocate per-layer scratch and emit the op lists.  grad_of maps id(param) -> tensor that
        receives its gradient (views of a flat buffer); required when training."""
        self._keep: List[torch.Tensor] = []       # tensors referenced only through raw pointers
        self._grad_of = grad_of
        if not self.training:
            self._compile_eval()
        elif self.bf16:
            self._compile_bf16(grad_of)
        else:
            self._compile_f32(grad_of)
        self.param_ptrs = self._signature()

    def _compile_eval(self):
        for r in self._convs():
            self._route_eval(r)
        rows: Dict[int, list] = defaultdict(list)
        self.fwd_ops = _pack(self._lower_forward(self._lower_conv_eval, rows))
        # BatchNorm folding + the transforms of the folded weights read only parameters and running statistics: they run once per
        # weight state (refresh_folded_weights), not once per forward -- at batch 1 the fold was the longest launch of the pass
        self.prep_ops = _pack(self._tables(rows))

    def _compile_f32(self, grad_of):
        # YH_GENERIC=1: every convolution on the generic gather-GEMM / wgrad kernels instead of the specialised families
        # (Winograd, pointwise, narrow, merged stride-2): the two are independent product paths that must agree
        # (tests/test_gpu_model.py::test_full_size_step_properties); the only planner switch besides YH_EVAL_FAST
        special = os.environ.get("YH_GENERIC", "0") != "1"
        firsts = self._pair_siblings(4)
        for r in self._convs():
            self._route_f32(r, special)
        for a in firsts:        # forward fusion of the siblings: one pointwise GEMM, N = cout1 + cout2
            a.fwd2 = a.pair.fwd2 = a.pw_f
        self._plan_fusion(special)
        rows: Dict[int, list] = defaultdict(list)
        fwd = self._lower_forward(self._lower_conv_f32, rows)
        self.fwd_ops = _pack(self._tables(rows) + rows[L.OP_PACK_WEIGHTS_S2M][::-1] + fwd)
        self.bwd_ops = _pack(self._lower_backward(grad_of))

    def _compile_bf16(self, grad_of):
        self._pair_siblings(8)
        for r in self._convs():
            self._route_bf16(r)
        rows: Dict[int, list] = defaultdict(list)
        fwd = self._lower_forward(self._lower_conv_bf16, rows)
        self.fwd_ops = _pack(self._tables(rows) + fwd)
        self.bwd_ops = _pack(self._lower_backward(grad_of))

    def _tables(self, rows: Dict[int, list]) -> List[L.YhOp]:
        """The weight transforms: each non-empty descriptor table packed into device memory, one *_MULTI launch per table."""
        ops = []
        for kind, fmt in _TABLES:
            if rows[kind]:
                t = torch.frombuffer(bytearray(b"".join(struct.pack(fmt, *d) for d in rows[kind])), dtype=torch.uint8).to(self.device)
                self._keep.append(t)
                ops.append(_op(kind, p=[t], i=[len(rows[kind])]))
        return ops

    def _lower_forward(self, lower_conv, rows: Dict[int, list]) -> List[L.YhOp]:
        """Records in trace order: fork / join markers, pools, and `lower_conv(ri, rec, fwd, rows)` for each convolution."""
        fwd: List[L.YhOp] = []
        for ri, r in enumerate(self.recs):
            if isinstance(r, SyncRec):
                if r.kind == "fork" and self._fork_deferred(ri + 1):
                    continue            # the fused sibling conv runs on the main lane; the fork follows its launch
                fwd.append(_op(L.OP_FORK if r.kind == "fork" else L.OP_JOIN))
            elif isinstance(r, ConvRec):
                lower_conv(ri, r, fwd, rows)
            elif not r.fused:
                self._lower_pool(ri, r, fwd)
        return fwd

    def _fork_deferred(self, ri: int) -> bool:
        r = self.recs[ri] if ri < len(self.recs) else None
        return isinstance(r, ConvRec) and r.fwd2 and r.pair_first and r.lane == 1

    def _lower_pool(self, ri: int, r: PoolRec, fwd: List[L.YhOp]):
        if not self.training and L.lib().yh_sppf_pool3_ok(r.x.H, r.x.W):
            # eval: SPPF's cascade pool5(pool5(pool5(x))) as one launch (no argmax, the plane stays in LDS)
            nxt = self.recs[ri + 1: ri + 3]
            if len(nxt) == 2 and all(isinstance(q, PoolRec) and q.lane == r.lane for q in nxt) \
                    and _same_view(nxt[0].x, r.out) and _same_view(nxt[1].x, nxt[0].out) \
                    and r.out.ld == nxt[0].out.ld == nxt[1].out.ld \
                    and all(v.ptr() % 16 == 0 for v in (r.out, nxt[0].out, nxt[1].out)):
                fwd.append(_op(L.OP_SPPF_POOL3, p=[r.x.ptr(), r.out.ptr(), nxt[0].out.ptr(), nxt[1].out.ptr()],
                               i=[r.x.ld, r.out.ld, r.x.B, r.x.H, r.x.W, r.x.C], lane=r.lane))
                nxt[0].fused = nxt[1].fused = True
                return
        r.arg = torch.empty(r.x.B, r.x.H, r.x.W, r.x.C, device=self.device, dtype=torch.uint8)
        fwd.append(_op(_OPS[self.bf16]["pool"], p=[r.x.ptr(), r.out.ptr(), r.arg], i=[r.x.ld, r.out.ld, r.x.B, r.x.H, r.x.W, r.x.C],
                       lane=r.lane))

    def _alloc_out(self, c: ConvRec, nblk: int, M: int):
        """Raw conv output, BatchNorm coefficients and partial-sum scratch (nblk rows from the forward kernel)."""
        if c.bn is not None and nblk <= 0:
            raise RuntimeError(f"planner: no forward block geometry for a {c.x.B}x{c.x.H}x{c.x.W} {c.cin}->{c.cout} convolution")
        c.nblk = nblk
        if c.bn is not None and c.coef is None:
            f32 = dict(device=self.device, dtype=torch.float32)
            c.y = torch.empty(c.x.B, c.Ho, c.Wo, c.cout, device=self.device, dtype=self.act_dtype)
            c.dyp, c.lddy = c.y.data_ptr(), c.cout
            if c.virtual:                         # the raw output lives in the output view itself (never normalised in memory)
                c.yp, c.ldy = c.out.ptr(), c.out.ld
            else:
                c.yp, c.ldy = c.dyp, c.lddy
            c.coef = torch.empty(4 * c.cout, **f32)
            c.part = torch.empty(max(nblk, L.lib().yh_bn_bwd_blocks(M, c.cout)) * 2 * c.cout, **f32)

    @staticmethod
    def _bn_finalize(r: ConvRec, M: int) -> L.YhOp:
        """Batch statistics from the forward's partial sums -> scale / shift in r.coef (and in the readers' prologue table when the
        output is virtual), running statistics updated."""
        bn = r.bn
        track = bn.track_running_stats and bn.running_mean is not None
        return _op(L.OP_BN_FINALIZE,
                   p=[r.part, bn.weight, bn.bias, bn.running_mean if track else None, bn.running_var if track else None, r.coef,
                      bn.num_batches_tracked if track else None,
                      r.out.icoef_ptr(0) if r.virtual else None, r.out.icoef_ptr(1) if r.virtual else None],
                   i=[r.nblk, r.cout], f=[bn.momentum if bn.momentum is not None else 0.1, bn.eps], l=[M], lane=r.lane)

    def _lower_conv_eval(self, ri: int, r: ConvRec, fwd: List[L.YhOp], rows: Dict[int, list]):
        """BatchNorm is folded into an OIHW copy of the weights (yh_fold_oihw_multi), which then goes through the weight transform
        of the layer's kernel family."""
        lib = L.lib()
        f32 = dict(device=self.device, dtype=torch.float32)
        bn, kk, cin_real = r.bn, r.k * r.k, r.weight.shape[1]
        fbias = torch.empty(r.cout, **f32)
        wfold = torch.empty(r.cout * cin_real * kk, **f32)
        self._keep += [fbias, wfold]
        rows[L.OP_FOLD_OIHW_MULTI].append(
            (r.weight.data_ptr(), r.bias.data_ptr() if r.bias is not None else 0, bn.weight.data_ptr() if bn is not None else 0,
             bn.bias.data_ptr() if bn is not None else 0, bn.running_mean.data_ptr() if bn is not None else 0,
             bn.running_var.data_ptr() if bn is not None else 0, wfold.data_ptr(), fbias.data_ptr(),
             r.cout, cin_real * kk, float(bn.eps) if bn is not None else 0.0, 0))
        l, extra = [], []
        if r.eval_fam == "lat":
            kind, r.wf = L.OP_CONV_LAT_FWD_FUSED, torch.zeros(kk * r.cin * r.ldwf, **f32)
            rows[L.OP_LAT_PACK_MULTI].append((wfold.data_ptr(), r.wf.data_ptr(), r.cout, cin_real, kk, r.ldwf))
        elif r.eval_fam == "wino":
            kind, r.wf = L.OP_CONV_WINO_FWD_FUSED, torch.empty(16 * r.cin * r.ldwf, **f32)
            rows[L.OP_WINO_WEIGHTS_MULTI].append((wfold.data_ptr(), r.wf.data_ptr(), r.cout, cin_real, r.ldwf, 0))
        elif r.eval_fam == "pw":
            kind, r.wf = L.OP_CONV_PW_FWD_FUSED, torch.zeros(r.cin * r.ldwf, **f32)
            rows[L.OP_PW_PACK_MULTI].append((wfold.data_ptr(), r.wf.data_ptr(), 0, r.cout, r.cin, r.ldwf, r.ldwb, 0, 0))
        else:
            kind, r.wf = L.OP_CONV_FWD_FUSED, torch.empty(kk * r.cin * r.ldwf, **f32)
            rows[L.OP_PACK_WEIGHTS_MULTI].append((wfold.data_ptr(), r.wf.data_ptr(), 0, r.cout, cin_real, kk, r.cin, r.ldwf, r.ldwb, 0, 0))
            nws = int(lib.yh_conv_fwd_fused_ws(r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s))
            sws = torch.zeros(nws, **f32) if nws > 0 else None   # per layer (two lanes may run split layers at once); zero tickets
            if sws is not None:
                self._keep.append(sws)
            l, extra = [nws], [sws]
        fwd.append(_op(kind, p=[r.x.ptr(), r.wf, fbias, r.residual.ptr() if r.residual else None, r.out.ptr()] + extra, l=l,
                       i=[r.x.ld, r.ldwf, r.residual.ld if r.residual else 0, r.out.ld, r.x.B, r.x.H, r.x.W,
                          r.cin, r.cout, r.k, r.s, int(bn is not None), int(r.upsample)], lane=r.lane))

    def _lower_conv_f32(self, ri: int, r: ConvRec, fwd: List[L.YhOp], rows: Dict[int, list]):
        lib = L.lib()
        f32 = dict(device=self.device, dtype=torch.float32)
        kk = r.k * r.k
        second = r.pair is not None and not r.pair_first
        # forward weights, in the layout of the forward's kernel family
        if r.fwd2 and second:
            pass                                      # shares its sibling's matrix
        elif r.pw_f:                                  # the pointwise pack writes only the conv's own columns
            if r.fwd2:
                r.ldwf = r.pair.ldwf = _rup4(r.cout + r.pair.cout)
            r.wf = torch.zeros(r.cin * r.ldwf, **f32)
            if r.fwd2:
                r.pair.wf = r.wf
        elif r.wino_f:
            r.wf = torch.empty(16 * r.cin * r.ldwf, **f32)
        elif r.s2l_f:
            r.wf = torch.zeros(kk * r.cin * r.ldwf, **f32)
        else:
            r.wf = torch.empty(kk * r.cin * r.ldwf, **f32)
        # backward-data weights
        if r.pair_first:          # stacked backward packs: rows [0, c1) this conv, [c1, c1 + c2) its sibling
            stacked = torch.empty((r.cout + r.pair.cout) * r.ldwb, **f32)
            if r.pw_b:            # one k-quad interleaved matrix for both: each record writes its own K rows
                r.wb = r.pair.wb = stacked
            else:
                r.wb, r.pair.wb = stacked[: r.cout * r.ldwb], stacked[r.cout * r.ldwb:]
            self._keep.append(stacked)
        elif r.s2m_b:
            r.ldwb = _rup4(2 * r.cin)
            r.wb = torch.empty(6 * r.cout * r.ldwb, **f32)
            rows[L.OP_PACK_WEIGHTS_S2M].append(_op(L.OP_PACK_WEIGHTS_S2M, p=[r.weight, r.wb], i=[r.cout, r.cin, r.ldwb]))
        elif r.need_dx and r.pair is None:
            # K rows of the backward pack: a 1x1 head reads dY rows zero-padded to a multiple of 4 channels against zero rows here
            r.kcout_b = _rup4(r.cout) if (r.bn is None and r.k == 1 and not (r.wino_b or r.pw_b) and r.out.ldg >= _rup4(r.cout)) else r.cout
            r.wb = (torch.zeros if r.kcout_b != r.cout else torch.empty)((16 if r.wino_b else kk) * r.kcout_b * r.ldwb, **f32)
        if r.pw_f or r.pw_b:
            rows[L.OP_PW_PACK_MULTI].append((r.weight.data_ptr(), r.wf.data_ptr() if r.pw_f else 0, r.wb.data_ptr() if r.pw_b else 0,
                                             r.cout, r.cin, r.ldwf, r.ldwb, r.pair.cout if second else 0,
                                             r.pair.cout if (second and r.fwd2) else 0))
        if r.wino_f:
            rows[L.OP_WINO_WEIGHTS_MULTI].append((r.weight.data_ptr(), r.wf.data_ptr(), r.cout, r.weight.shape[1], r.ldwf, 0))
        if r.wino_b:
            rows[L.OP_WINO_WEIGHTS_MULTI].append((r.weight.data_ptr(), r.wb.data_ptr(), r.cout, r.weight.shape[1], r.ldwb, 1))
        if r.s2l_f:
            rows[L.OP_LAT_PACK_MULTI].append((r.weight.data_ptr(), r.wf.data_ptr(), r.cout, r.weight.shape[1], kk, r.ldwf))
        gen_f = not (r.wino_f or r.pw_f or r.s2l_f)            # layouts the generic pack kernel still has to write
        gen_b = r.wb is not None and not (r.wino_b or r.pw_b or r.s2m_b)
        if gen_f or gen_b:
            rows[L.OP_PACK_WEIGHTS_MULTI].append((r.weight.data_ptr(), r.wf.data_ptr() if gen_f else 0, r.wb.data_ptr() if gen_b else 0,
                                                  r.cout, r.weight.shape[1], kk, r.cin, r.ldwf, r.ldwb, 0, 0))
        M = r.x.B * r.Ho * r.Wo
        if r.fwd2:
            if r.pair_first:      # both siblings in one launch, at the first one's position in the list
                q = r.pair
                nblk = lib.yh_conv_pw_blocks(M, r.cin, r.cout + q.cout)
                self._alloc_out(r, nblk, M)
                self._alloc_out(q, nblk, M)
                # on the main lane whatever lane the record was traced on: both siblings' BN passes depend on it
                fwd.append(_op(L.OP_CONV_PW_FWD2, p=[r.x.ptr(), r.wf, r.bias, r.yp, r.part, q.bias, q.yp, q.part],
                               i=[r.x.ld, r.ldwf, r.ldy, r.x.B, r.x.H, r.x.W, r.cin, r.cout, q.ldy, q.cout], lane=0))
                if r.x_fused:
                    _set_prologue(fwd[-1], r.x)
                prev = self.recs[ri - 1] if ri else None
                if r.lane == 1 and isinstance(prev, SyncRec) and prev.kind == "fork":
                    fwd.append(_op(L.OP_FORK))        # deferred by _lower_forward
                elif r.lane == 1 or q.lane == 1:
                    raise NotImplementedError("fused sibling convolution traced on the side lane without a preceding fork")
        else:
            nblk = lib.yh_conv_narrow_blocks(r.x.B, r.x.H, r.x.W, r.cin, r.s) if r.narrow_f else \
                lib.yh_conv_s2_blocks(r.x.B, r.x.H, r.x.W, r.cout) if r.s2l_f else \
                lib.yh_conv_wino_blocks(r.x.B, r.x.H, r.x.W) if r.wino_f else \
                lib.yh_conv_pw_blocks(M, r.cin, r.cout) if r.pw_f else \
                lib.yh_conv_fwd_blocks(r.x.B, r.x.H, r.x.W, r.cout, r.k, r.s)
            self._alloc_out(r, nblk, M)
            yt, ldy = (r.yp, r.ldy) if r.bn is not None else (r.out.ptr(), r.out.ld)
            p = [r.x.ptr(), r.wf, r.bias, yt, r.part if r.bn is not None else None]
            if r.narrow_f:
                fwd.append(_op(L.OP_CONV_NARROW, p=p, i=[r.x.ld, r.ldwf, ldy, r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.s, 0, 0], lane=r.lane))
            else:
                kind = L.OP_CONV_S2_FWD if r.s2l_f else L.OP_CONV_WINO_FWD if r.wino_f else L.OP_CONV_PW_FWD if r.pw_f else L.OP_CONV_FWD
                fwd.append(_op(kind, p=p, i=[r.x.ld, r.ldwf, ldy, r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s], lane=r.lane))
            if r.x_fused:                             # the input's BatchNorm + SiLU is applied while this kernel stages it
                _set_prologue(fwd[-1], r.x)
        if r.bn is not None:
            fwd.append(self._bn_finalize(r, M))
            if not r.virtual:
                rf = self._res_fused(r)               # the residual is a raw conv output: normalised on the fly
                fwd.append(_op(L.OP_BN_SILU_FWD,
                               p=[r.yp, r.coef, r.residual.ptr() if r.residual else None, r.out.ptr(),
                                  r.residual.icoef_ptr() if rf else None],
                               i=[r.ldy, r.residual.ld if r.residual else 0, r.out.ld, r.cout, r.Ho, r.Wo,
                                  int(r.upsample), r.residual.icoef_ld if rf else 0], l=[M], lane=r.lane))

    def _lower_conv_bf16(self, ri: int, r: ConvRec, fwd: List[L.YhOp], rows: Dict[int, list]):
        lib = L.lib()
        b16 = dict(device=self.device, dtype=torch.bfloat16)
        kk, cin_real = r.k * r.k, r.weight.shape[1]
        r.wf = torch.empty(kk * r.cin * r.ldwf, **b16)
        kpad, koff = _rup8(r.cout), 0
        if r.need_dx:
            if r.pair is not None:
                kpad = r.cout + r.pair.cout
                if r.pair_first:
                    r.wb = r.pair.wb = torch.zeros(kpad * r.ldwb, **b16)
                else:
                    koff = r.pair.cout
            else:
                r.wb = torch.zeros(kk * kpad * r.ldwb, **b16)
        rows[L.OP_BF16_PACK_MULTI].append((r.weight.data_ptr(), r.wf.data_ptr(), r.wb.data_ptr() if r.need_dx else 0, r.cout, cin_real,
                                           kk, r.cin, r.ldwf, r.ldwb, koff, kpad))
        M = r.x.B * r.Ho * r.Wo
        self._alloc_out(r, lib.yh_conv_narrow_blocks(r.x.B, r.x.H, r.x.W, r.cin_k, r.s) if r.narrow_f else
                        lib.yh_bf16_conv_fwd_blocks(r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s, 0 if r.bn is not None else 1, r.x.ld,
                                                    r.cout if r.bn is not None else r.out.ld), M)
        if r.bn is None:        # head output: fp32, no BatchNorm
            fwd.append(_op(L.OP_BF16_CONV_FWD, p=[r.x.ptr(), r.wf, r.bias, r.out.ptr(), None],
                           i=[r.x.ld, r.ldwf, r.out.ld, r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s, 1], lane=r.lane))
            return
        if r.narrow_f:
            fwd.append(_op(L.OP_BF16_CONV_NARROW, p=[r.x.ptr(), r.wf, r.bias, r.yp, r.part],
                           i=[r.x.ld, r.ldwf, r.ldy, r.x.B, r.x.H, r.x.W, r.cin_k, r.cout, r.s, 0, 0, r.cin], lane=r.lane))
        else:
            fwd.append(_op(L.OP_BF16_CONV_FWD, p=[r.x.ptr(), r.wf, r.bias, r.yp, r.part],
                           i=[r.x.ld, r.ldwf, r.ldy, r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s, 0], lane=r.lane))
        fwd.append(self._bn_finalize(r, M))
        fwd.append(_op(L.OP_BF16_BN_SILU_FWD, p=[r.yp, r.coef, r.residual.ptr() if r.residual else None, r.out.ptr()],
                       i=[r.ldy, r.residual.ld if r.residual else 0, r.out.ld, r.cout, r.Ho, r.Wo, int(r.upsample)], l=[M], lane=r.lane))

    def _grad_target(self, v: View) -> Tuple[int, int]:
        """Pointer into the gradient tensor of `v` and whether the op must accumulate."""
        cov = v.buf.grad_cover
        lo, hi = v.off, v.off + v.C
        inside = any(a <= lo and hi <= b for a, b in cov)
        overlap = any(a < hi and lo < b for a, b in cov)
        if inside:
            return v.gptr(), 1
        if overlap:
            raise NotImplementedError(f"partial gradient overlap on buffer {v.buf.name}")
        cov.append((lo, hi))
        return v.gptr(), 0

    def _wgrad_ws(self, r: ConvRec) -> int:
        lib = L.lib()
        if r.narrow_w:
            return lib.yh_conv_narrow_bwd_weight_ws(r.x.B, r.x.H, r.x.W, r.cin_k, r.cout, r.s)
        if r.wino_w:
            return lib.yh_conv_wino_bwd_weight_ws(r.x.B, r.x.H, r.x.W, r.cin, r.cout)
        if r.pw_w:
            return lib.yh_conv_pw_bwd_weight_ws(r.x.B * r.x.H * r.x.W, r.cin, r.cout)
        return (lib.yh_bf16_conv_bwd_weight_ws if self.bf16 else lib.yh_conv_bwd_weight_ws)(r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s)

    def _lower_backward(self, grad_of) -> List[L.YhOp]:
        """The records in reverse: BatchNorm + SiLU backward (dY over Y), bias and weight gradients, backward-data into the input's
        gradient (written or accumulated, see _grad_target).  One walk for fp32 and bf16 plans; _OPS holds the per-type op kinds."""
        lib = L.lib()
        K = _OPS[self.bf16]
        if grad_of is None:
            raise ValueError("training plan needs gradient destinations")
        for b in self.buffers:
            b.grad_cover = []
        # gradients of the declared outputs arrive from outside (loss kernel / autograd) fully written
        for v, _ in self.outputs:
            v.buf.grad_cover.append((v.off, v.off + v.C))
        ws_floats = 1
        for r in self._convs():
            ws_floats = max(ws_floats, self._wgrad_ws(r))
            if r.bias is not None:
                ws_floats = max(ws_floats, lib.yh_colsum_ws(r.x.B * r.Ho * r.Wo, r.cout))
        self.ws = torch.empty(int(ws_floats), device=self.device, dtype=torch.float32)
        ops: List[L.YhOp] = []
        pair_pending = set()
        self.grad_ready: Dict[int, int] = {}     # id(param) -> number of backward ops after which its grad is final
        for r in reversed(self.recs):
            if isinstance(r, SyncRec):
                continue
            if isinstance(r, PoolRec):
                dst, acc = self._grad_target(r.x)
                if not acc:
                    raise NotImplementedError("max-pool backward expects an already written input gradient")
                ops.append(_op(K["pool_bwd"], p=[r.out.gptr(), r.arg, dst], i=[r.out.ldg, r.x.ldg, r.x.B, r.x.H, r.x.W, r.x.C]))
                continue
            M = r.x.B * r.Ho * r.Wo
            if r.bn is not None:
                nb = lib.yh_bn_bwd_blocks(M, r.cout)
                ops.append(_op(K["reduce"], p=[r.out.gptr(), r.yp, r.coef, r.part], i=[r.out.ldg, r.ldy, r.cout, r.Ho, r.Wo, int(r.upsample)],
                               l=[M]))
                dres, racc = self._grad_target(r.residual) if r.residual is not None else (None, 0)
                ops.append(_op(K["apply"],
                               p=[r.out.gptr(), r.yp, r.coef, r.part, r.bn.weight, grad_of[id(r.bn.weight)], grad_of[id(r.bn.bias)],
                                  r.dyp, dres],
                               i=[r.out.ldg, r.ldy, nb, r.lddy, r.residual.ldg if r.residual is not None else 0, racc, r.cout, r.Ho,
                                  r.Wo, int(r.upsample)], l=[M]))
                dy, lddy, kcout = r.dyp, r.lddy, r.cout
                self.grad_ready[id(r.bn.weight)] = self.grad_ready[id(r.bn.bias)] = len(ops)
            else:       # head: the loss / autograd wrote rows zero-padded to ldg channels
                dy, lddy, kcout = r.out.gptr(), r.out.ldg, r.kcout_b or r.cout
            fuse_bias = r.bias is not None and r.narrow_w          # the narrow weight-gradient kernel also sums dY's columns
            if r.bias is not None and not fuse_bias:
                # head biases: sum the zero-padded multiple of 4 so the vector kernel applies; the extra column sums are exact zeros
                # and land in the 4-float padding every tensor has in the flat gradient buffer
                cs = _rup4(r.cout) if (r.bn is None and _rup4(r.cout) <= lddy) else r.cout
                ops.append(_op(K["colsum"], p=[dy, grad_of[id(r.bias)], self.ws], i=[lddy, cs], l=[M]))
                self.grad_ready[id(r.bias)] = len(ops)
            cin, cin_real = (r.cin_k, min(r.weight.shape[1], r.cin_k)) if r.narrow_w else (r.cin, r.weight.shape[1])
            ops.append(_op(K["narrow_w"] if r.narrow_w else L.OP_CONV_WINO_BWD_WEIGHT if r.wino_w else
                           L.OP_CONV_PW_BWD_WEIGHT if r.pw_w else K["wgrad"],
                           p=[r.x.ptr(), dy, grad_of[id(r.weight)], self.ws, grad_of[id(r.bias)] if fuse_bias else None],
                           i=[r.x.ld, lddy, r.x.B, r.x.H, r.x.W, cin, cin_real, r.cout, r.k, r.s], l=[self.ws.numel()]))
            if r.x_fused:                                          # x is a raw conv output: the kernel normalises it while staging
                _set_prologue(ops[-1], r.x)
            self.grad_ready[id(r.weight)] = len(ops)
            if fuse_bias:
                self.grad_ready[id(r.bias)] = len(ops)
            if not r.need_dx:
                continue
            if r.pair is not None and id(r.pair) not in pair_pending:
                pair_pending.add(id(r))                             # first of the pair in backward order: wait for the sibling's dY
                continue
            dst, acc = self._grad_target(r.x)
            kpad = [_rup8(r.cout)] if self.bf16 else []             # bf16 narrow kernels: K rows of the backward pack
            if r.pair is not None:                                  # both siblings' dY are final now: one GEMM over K = c1 + c2
                a, b = (r, r.pair) if r.pair_first else (r.pair, r)
                if self.bf16:
                    ops.append(_op(L.OP_BF16_CONV_BWD_DATA, p=[a.y, a.wb, dst, b.y],
                                   i=[a.cout, a.ldwb, r.x.ldg, r.x.B, r.x.H, r.x.W, r.cin, a.cout + b.cout, 1, 1, acc, a.cout]))
                else:
                    ops.append(_op(L.OP_CONV_PW_BWD_DATA if r.pw_b else L.OP_CONV_BWD_DATA_PAIR, p=[a.y, b.y, a.wb, dst],
                                   i=[a.cout, b.cout, a.cout, a.ldwb, r.x.ld, r.x.B, r.x.H, r.x.W, r.cin, acc]))
            elif r.narrow_b and r.s == 2:
                ops.append(_op(K["narrow_s2"], p=[dy, r.wb, dst],
                               i=[lddy, r.ldwb, r.x.ldg, r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s, acc] + kpad))
            elif r.narrow_b:     # x = dY (Cout channels), output = dX (Cin channels), backward pack, flipped taps
                ops.append(_op(K["narrow"], p=[dy, r.wb, None, dst, None],
                               i=[lddy, r.ldwb, r.x.ldg, r.x.B, r.x.H, r.x.W, r.cout, r.cin, 1, 1, acc] + kpad))
            elif r.s2m_b:
                ops.append(_op(L.OP_CONV_BWD_DATA_S2M, p=[dy, r.wb, dst],
                               i=[lddy, r.ldwb, r.x.ld, r.x.B, r.x.H, r.x.W, r.cin, r.cout, r.k, r.s, acc]))
            elif r.pw_b:
                ops.append(_op(L.OP_CONV_PW_BWD_DATA, p=[dy, None, r.wb, dst],
                               i=[r.cout, 0, lddy, r.ldwb, r.x.ld, r.x.B, r.x.H, r.x.W, r.cin, acc]))
            elif r.wino_b:
                ops.append(_op(L.OP_CONV_WINO_BWD_DATA, p=[dy, r.wb, dst],
                               i=[lddy, r.ldwb, r.x.ld, r.x.B, r.x.H, r.x.W, r.cin, r.cout, acc]))
            else:
                ops.append(_op(K["dgrad"], p=[dy, r.wb, dst],
                               i=[lddy, r.ldwb, r.x.ldg, r.x.B, r.x.H, r.x.W, r.cin, kcout, r.k, r.s, acc]))
        # (folding the BatchNorm-backward sums into the epilogue of the backward-data GEMM that finishes a layer's gradient was
        # built, tested and measured in round 2: backward-data 5.74 -> 7.26 ms against 0.85 ms saved in the reduce pass; retired)
        return ops

    # ---- execution ----------------------------------------------------------------------------
    def _signature(self) -> List[int]:
        """Every device address the op lists bake in that the plan does not own: parameters, BatchNorm buffers
        (running statistics, num_batches_tracked) and the gradient destinations."""
        if self._sig_holders is None:       # (module, attribute) pairs: `bn.running_mean = t` / `p.data = t` must be seen
            hold, seen = [], set()
            for r in self.recs:
                if not isinstance(r, ConvRec):
                    continue
                if id(r.conv) not in seen:
                    seen.add(id(r.conv))
                    hold += [(r.conv, "weight"), (r.conv, "bias")]
                if r.bn is not None and id(r.bn) not in seen:
                    seen.add(id(r.bn))
                    hold += [(r.bn, "weight"), (r.bn, "bias"), (r.bn, "running_mean"), (r.bn, "running_var"),
                             (r.bn, "num_batches_tracked")]
            self._sig_holders = hold
        sig: List[int] = []
        for obj, attr in self._sig_holders:
            t = getattr(obj, attr)
            if t is None:
                sig.append(0)
                continue
            sig.append(t.data_ptr())
            if self._grad_of:
                g = self._grad_of.get(id(t))
                sig.append(g.data_ptr() if g is not None else 0)
        return sig

    def params_moved(self) -> bool:
        """True when a parameter, BatchNorm buffer or gradient destination no longer lives at the address the op
        lists hold (HipTrainer moved the parameters into its flat buffer, load_state_dict(assign=True), a
        reassigned running_mean, ...): the plan must be re-traced, a captured hipGraph re-captured."""
        return self._signature() != self.param_ptrs

    def _ctx(self):
        """This thread's execution context for the plan's device (the C side refuses a context on a foreign device)."""
        return L.context_for(self.device.index if self.device.index is not None else torch.cuda.current_device())

    def _on_device(self):
        dev = self.device.index
        return torch.cuda.device(dev) if dev is not None and torch.cuda.current_device() != dev else _NullCtx()

    def weights_state(self):
        """What the folded inference weights were computed from: the process-wide counter of in-place updates made by this
        package's own kernels (which write through raw pointers and so bypass torch's version counters: optimizer steps,
        BatchNorm running statistics of training forwards) plus torch's version counter of every tensor the fold reads."""
        if self._fold_tensors is None:
            self._signature()
            self._fold_tensors = [(o, a) for o, a in self._sig_holders if a != "num_batches_tracked"]
        v = 0
        for o, a in self._fold_tensors:
            t = getattr(o, a)
            if t is not None:
                v += t._version
        return (WEIGHTS_EPOCH[0], v)

    def fold_inputs(self) -> List[torch.Tensor]:
        """The tensors the fold reads, resolved once (InferenceSession sums their version counters per image without
        walking the module tree; a re-assigned attribute shows up as a PARAM_GENERATION / signature change instead)."""
        self.weights_state()
        return [t for t in (getattr(o, a) for o, a in self._fold_tensors) if t is not None]

    def refresh_folded_weights(self, stream: int) -> bool:
        """Eval plans: (re)fold BatchNorm into the packed weights when the weights changed since the last fold."""
        if self.prep_ops is None:
            return False
        state = self.weights_state()
        if state == self._folded_state:
            return False
        with self._on_device():
            L.run_ops(self.prep_ops[0], self.prep_ops[1], stream, None)
        self._folded_state = state
        return True

    def run_forward(self, stream: int):
        if self.training:
            WEIGHTS_EPOCH[0] += 1          # running statistics / num_batches_tracked are about to change under torch's radar
        else:
            self.refresh_folded_weights(stream)
        with self._on_device():
            L.run_ops(self.fwd_ops[0], self.fwd_ops[1], stream, self._ctx())
        self.generation += 1

    def run_backward(self, stream: int, begin: int = 0, end: Optional[int] = None):
        """Run backward ops [begin, end) (the trainer splits the list at gradient-bucket boundaries)."""
        arr, n = self.bwd_ops
        end = n if end is None else end
        if end > begin:
            with self._on_device():
                L.run_ops(ctypes.cast(ctypes.byref(arr, begin * ctypes.sizeof(L.YhOp)), ctypes.POINTER(L.YhOp)), end - begin,
                          stream, self._ctx())


class _NullCtx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def _addr(x) -> Optional[int]:
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


def _op(kind: int, p=(), i=(), f=(), l=(), lane: int = 0) -> L.YhOp:
    o = L.YhOp()
    o.kind = kind
    o.lane = lane
    for n, v in enumerate(p):
        o.p[n] = _addr(v)
    for n, v in enumerate(i):
        o.i[n] = int(v)
    for n, v in enumerate(f):
        o.f[n] = float(v)
    for n, v in enumerate(l):
        o.l[n] = int(v)
    return o


def _set_prologue(o: L.YhOp, x: "View"):
    """Convolution records carry the input-prologue table of their x operand in p[10] and its row stride in i[17]."""
    o.p[10] = x.icoef_ptr()
    o.i[17] = x.icoef_ld


def _pack(ops: List[L.YhOp]):
    arr = (L.YhOp * max(len(ops), 1))()
    for n, o in enumerate(ops):
        arr[n] = o
    return arr, len(ops)
