"""The input prologue (z = x * scale + shift, silu(z) where gate != 0, zero padding after the activation) of every `_act` entry
point, of the residual reader yh_bn_silu_fwd_res and of the table writer yh_bn_finalize_x, against a float64 evaluation.

Every convolution case runs as a one-record op list through yh_run, so api.hip's slot mapping (p[10] / i[17]) is covered with
the kernel.  Two groups of cases:
  - edge cases at reduced size, one group per entry point: gates mixed inside a 4-channel quad and the concatenation pattern
    (a SiLU half next to an identity half), shifts up to |3| (prologue(0) != 0, so a halo activated before masking shows at
    every border pixel), one saturating channel (z ~ +-100), a table view at a non-zero offset with NaN outside it, input
    views with ld > C and NaN outside them, output views with a sentinel outside them that must survive;
  - a sweep over every prologue launch of four training plans (compiled on the CPU, as tools/plan_dump.py does) at full batch
    and resolution, with each record's own ld's, offsets and gate row.
Tolerances (relative to max |ref|): forward outputs and BatchNorm partial sums 1e-5, pointwise weight gradient at reduced size
1e-5, every other weight gradient 1e-4."""
import ctypes
import struct
import zlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SENT = -7777.0          # sentinel outside every output view
FWD_TOL, PART_TOL, WGRAD_TOL, PW_WGRAD_TOL = 1e-5, 1e-5, 1e-4, 1e-5


def _lib():
    import yolo_from_scratch_amd._lib as L
    return L


def rup4(c):
    return (c + 3) // 4 * 4


# ---- float64 reference: convolution as k*k shifted GEMMs (any device) ------------------------------------------------------------

def prologue64(x, tab):
    """x: NHWC; tab: (3, C) rows [scale | shift | gate]; float64 result."""
    x, tab = x.double(), tab.double()
    z = x * tab[0] + tab[1]
    return torch.where(tab[2] != 0, z * torch.sigmoid(z), z)


def _taps(x, k, s):
    """Zero-padded (after any prologue) NHWC input -> the k*k shifted views, each (B, Ho, Wo, C)."""
    p = k // 2
    B, H, W, _ = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = F.pad(x, (0, 0, p, p, p, p))
    for kh in range(k):
        for kw in range(k):
            yield kh, kw, xp[:, kh: kh + s * (Ho - 1) + 1: s, kw: kw + s * (Wo - 1) + 1: s, :]


def conv_fwd64(x, w, bias=None, s=1, tab=None):
    """NHWC x, OIHW w -> NHWC float64 output of the k x k, stride s, pad k // 2 convolution of prologue(x)."""
    x = prologue64(x, tab) if tab is not None else x.double()
    w = w.double()
    y = None
    for kh, kw, xs in _taps(x, w.shape[-1], s):
        t = torch.matmul(xs, w[:, :, kh, kw].t())
        y = t if y is None else y.add_(t)
    return y if bias is None else y + bias.double()


def conv_wgrad64(x, dy, k, s=1, tab=None):
    """NHWC x, NHWC dy -> OIHW float64 weight gradient of the same convolution."""
    x = prologue64(x, tab) if tab is not None else x.double()
    d = dy.double().reshape(-1, dy.shape[-1]).t()
    dw = torch.empty(dy.shape[-1], x.shape[-1], k, k, dtype=torch.float64, device=x.device)
    for kh, kw, xs in _taps(x, k, s):
        dw[:, :, kh, kw] = d @ xs.reshape(-1, x.shape[-1])
    return dw


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s", [(2, 7, 9, 5, 6, 3, 1), (3, 9, 7, 4, 3, 3, 2), (2, 5, 11, 6, 7, 1, 1),
                                                 (2, 8, 6, 3, 5, 3, 2), (1, 6, 6, 4, 4, 1, 2)])
def test_fp64_reference_matches_torch(B, H, W, Cin, Cout, k, s):
    """The reference itself, on every machine: forward and weight gradient against F.conv2d / conv2d_weight in float64, with and
    without the prologue."""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + Cin)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    tab = torch.stack([torch.rand(Cin, generator=g, dtype=torch.float64) + 0.5, torch.randn(Cin, generator=g, dtype=torch.float64) * 2,
                       (torch.arange(Cin) % 3 != 0).double()])
    for t in (None, tab):
        xa = (prologue64(x, t) if t is not None else x).permute(0, 3, 1, 2)
        ref = F.conv2d(xa, w, bias, stride=s, padding=k // 2)
        got = conv_fwd64(x, w, bias, s, t).permute(0, 3, 1, 2)
        assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())
        dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
        dref = torch.nn.grad.conv2d_weight(xa, w.shape, dy, stride=s, padding=k // 2)
        dgot = conv_wgrad64(x, dy.permute(0, 2, 3, 1), k, s, t)
        assert float((dgot - dref).abs().max()) < 1e-12 * float(dref.abs().max())
    z = torch.tensor([0.0, -3.0, 2.5], dtype=torch.float64)[None, None, None, :]
    t = torch.tensor([[1.0, 1.0, 1.0], [0.5, -3.0, 2.5], [1.0, 1.0, 0.0]], dtype=torch.float64)
    p = prologue64(z, t).flatten()                       # silu(0.5), silu(-6), identity (2.5 * 1 + 2.5)
    assert torch.allclose(p, torch.tensor([0.5 / (1 + np.exp(-0.5)), -6 / (1 + np.exp(6)), 5.0], dtype=torch.float64))


# ---- one case of one family: shapes, views, table, and how it ran in the plan ----------------------------------------------------

FWD_KINDS = ("OP_CONV_FWD", "OP_CONV_S2_FWD", "OP_CONV_WINO_FWD", "OP_CONV_PW_FWD", "OP_CONV_NARROW", "OP_CONV_PW_FWD2")
WGRAD_KINDS = ("OP_CONV_BWD_WEIGHT", "OP_CONV_WINO_BWD_WEIGHT", "OP_CONV_PW_BWD_WEIGHT", "OP_CONV_NARROW_BWD_WEIGHT")
ACT_KINDS = FWD_KINDS + WGRAD_KINDS


@dataclass(frozen=True)
class Case:
    kind: str
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int = 3
    s: int = 1
    cin_real: int = 0                 # weight gradients: real input channels (0: Cin)
    ldx: int = 0                      # input view (0: Cin, offset 0)
    xoff: int = 0
    tld: int = 0                      # table stride (0: rup4(ldx) + 4, as graph.Buffer.icoef); the table view starts at xoff
    ldy: int = 0                      # output view (forward) / dY view (weight gradients)
    yoff: int = 0
    cout2: int = 0                    # OP_CONV_PW_FWD2: second output
    ldy2: int = 0
    y2off: int = 0
    bias: bool = False
    part: bool = True                 # forward: BatchNorm partial sums
    dbias: bool = False               # OP_CONV_NARROW_BWD_WEIGHT: bias gradient
    gate: Tuple[int, ...] = ()        # gate row of the table (() = c % 3 != 0)
    sat: int = 1                      # saturating channel (scale 40), -1 = none
    i: Tuple[int, ...] = ()           # integer slots of the plan's record ( (): built here in graph.py's layout)

    def __post_init__(self):
        d = dict(ldx=self.ldx or self.Cin, ldy=self.ldy or self.Cout, cin_real=self.cin_real or self.Cin)
        d["tld"] = self.tld or rup4(d["ldx"]) + 4
        if self.kind == "OP_CONV_PW_FWD2":
            d["ldy2"] = self.ldy2 or self.cout2
        if not self.gate:
            d["gate"] = tuple(int(c % 3 != 0) for c in range(self.Cin))
        for k2, v in d.items():
            object.__setattr__(self, k2, v)

    @property
    def Ho(self):
        return (self.H + 2 * (self.k // 2) - self.k) // self.s + 1

    @property
    def Wo(self):
        return (self.W + 2 * (self.k // 2) - self.k) // self.s + 1

    def name(self):
        ex = f"+{self.cout2}" if self.cout2 else ""
        return (f"{self.kind[3:].lower()}-{self.B}x{self.H}x{self.W}-{self.Cin}to{self.Cout}{ex}-k{self.k}s{self.s}"
                f"-ldx{self.ldx}o{self.xoff}-ldy{self.ldy}o{self.yoff}")


def make_table(C, tld, toff, gate, sat, gen, device, big_shift=3.0):
    """(3, tld) table with NaN outside the view [toff, toff + C); scale in [0.25, 1.75], |shift| up to big_shift, one channel
    with scale 40 (z ~ +-100 at x ~ N(0, 1))."""
    t = torch.full((3, tld), float("nan"), device=device)
    sc = torch.rand(C, generator=gen, device=device) * 1.5 + 0.25
    sh = (torch.rand(C, generator=gen, device=device) * 2 - 1) * big_shift
    if 0 <= sat < C:
        sc[sat] = 40.0
    t[0, toff:toff + C], t[1, toff:toff + C] = sc, sh
    t[2, toff:toff + C] = torch.tensor(gate, dtype=torch.float32, device=device)
    return t


def view_buf(shape_px, ld, off, C, gen, device, outside=float("nan")):
    """(…, ld) buffer: random N(0, 1) in channels [off, off + C), `outside` elsewhere."""
    buf = torch.full(tuple(shape_px) + (ld,), outside, device=device)
    buf[..., off:off + C] = torch.randn(tuple(shape_px) + (C,), generator=gen, device=device)
    return buf


def _seed(text):
    return zlib.crc32(text.encode()) % 100003


def rel_err(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


def part_err(part, ref, C):
    """Partial sums [nblk][2][C] against the fp64 sums of the output (relative to the largest per-channel |sum|)."""
    s = part.view(-1, 2, C).double().sum(0)
    r = ref.reshape(-1, C)
    e0 = (s[0] - r.sum(0)).abs().max() / r.abs().sum(0).max()
    e1 = (s[1] - (r * r).sum(0)).abs().max() / (r * r).sum(0).max()
    return float(max(e0, e1))


def _desc(fmt, *vals, device="cuda"):
    return torch.frombuffer(bytearray(struct.pack(fmt, *vals)), dtype=torch.uint8).to(device)


def _record(L, kind, i, p, l=()):
    o = L.YhOp()
    o.kind = getattr(L, kind)
    for n, v in enumerate(i):
        o.i[n] = int(v)
    for n, v in enumerate(p):
        o.p[n] = v or None
    for n, v in enumerate(l):
        o.l[n] = int(v)
    return o


def _run1(L, o):
    arr = (L.YhOp * 1)(o)
    L.run_ops(arr, 1, torch.cuda.current_stream().cuda_stream)


def _nblk(lib, c):
    M = c.B * c.Ho * c.Wo
    return {"OP_CONV_NARROW": lambda: lib.yh_conv_narrow_blocks(c.B, c.H, c.W, c.Cin, c.s),
            "OP_CONV_S2_FWD": lambda: lib.yh_conv_s2_blocks(c.B, c.H, c.W, c.Cout),
            "OP_CONV_WINO_FWD": lambda: lib.yh_conv_wino_blocks(c.B, c.H, c.W),
            "OP_CONV_PW_FWD": lambda: lib.yh_conv_pw_blocks(M, c.Cin, c.Cout),
            "OP_CONV_PW_FWD2": lambda: lib.yh_conv_pw_blocks(M, c.Cin, c.Cout + c.cout2),
            "OP_CONV_FWD": lambda: lib.yh_conv_fwd_blocks(c.B, c.H, c.W, c.Cout, c.k, c.s)}[c.kind]()


def _ws_floats(lib, c):
    return {"OP_CONV_BWD_WEIGHT": lambda: lib.yh_conv_bwd_weight_ws(c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.s),
            "OP_CONV_WINO_BWD_WEIGHT": lambda: lib.yh_conv_wino_bwd_weight_ws(c.B, c.H, c.W, c.Cin, c.Cout),
            "OP_CONV_PW_BWD_WEIGHT": lambda: lib.yh_conv_pw_bwd_weight_ws(c.B * c.H * c.W, c.Cin, c.Cout),
            "OP_CONV_NARROW_BWD_WEIGHT": lambda: lib.yh_conv_narrow_bwd_weight_ws(c.B, c.H, c.W, c.Cin, c.Cout, c.s)}[c.kind]()


def _pack_fwd(L, lib, c, w, w2, st):
    """The forward weight pack of the family, written by the same entry point the plan's prep ops use, at the record's ldw."""
    kk, dev = c.k * c.k, w.device
    ldw = c.i[1] if c.i else rup4(c.Cout + c.cout2)
    assert ldw >= c.Cout + c.cout2
    if c.kind == "OP_CONV_WINO_FWD":
        wf = torch.full((16 * c.Cin * ldw,), float("nan"), device=dev)
        L.check(lib.yh_wino_weights_multi(_desc("<QQiiii", w.data_ptr(), wf.data_ptr(), c.Cout, c.Cin, ldw, 0).data_ptr(), 1, st))
    elif c.kind == "OP_CONV_S2_FWD":
        wf = torch.zeros(kk * c.Cin * ldw, device=dev)
        L.check(lib.yh_lat_pack_multi(_desc("<QQiiii", w.data_ptr(), wf.data_ptr(), c.Cout, c.Cin, kk, ldw).data_ptr(), 1, st))
    elif c.kind in ("OP_CONV_PW_FWD", "OP_CONV_PW_FWD2"):
        wf = torch.zeros(c.Cin * ldw, device=dev)
        rows = [(w, c.Cout, 0)] + ([(w2, c.cout2, c.Cout)] if c.cout2 else [])
        d = b"".join(struct.pack("<QQQiiiiii", ww.data_ptr(), wf.data_ptr(), 0, co, c.Cin, ldw, rup4(c.Cin), noff, noff)
                     for ww, co, noff in rows)
        L.check(lib.yh_pw_pack_multi(torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev).data_ptr(), len(rows), st))
    else:                                                   # gather GEMM and narrow kernel: the generic pack
        wf = torch.full((kk * c.Cin * ldw,), float("nan"), device=dev)
        L.check(lib.yh_pack_weights_multi(_desc("<QQQiiiiiiii", w.data_ptr(), wf.data_ptr(), 0, c.Cout, c.Cin, kk, c.Cin, ldw,
                                                rup4(c.Cin), 0, 0).data_ptr(), 1, st))
    torch.cuda.synchronize()
    return wf, ldw


def _fwd_slots(c, ldw):
    if c.kind == "OP_CONV_NARROW":
        return [c.ldx, ldw, c.ldy, c.B, c.H, c.W, c.Cin, c.Cout, c.s, 0, 0]
    if c.kind == "OP_CONV_PW_FWD2":
        return [c.ldx, ldw, c.ldy, c.B, c.H, c.W, c.Cin, c.Cout, c.ldy2, c.cout2]
    return [c.ldx, ldw, c.ldy, c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.s]


def _with_table(i, tld):
    i = list(i) + [0] * (19 - len(i))
    i[17] = tld
    return i


def run_forward(c: Case, seed: int, fwd_tol=FWD_TOL, part_tol=PART_TOL):
    L = _lib()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    xb = view_buf((c.B, c.H, c.W), c.ldx, c.xoff, c.Cin, g, dev)
    tab = make_table(c.Cin, c.tld, c.xoff, c.gate, c.sat, g, dev)
    w = torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g, device=dev) / (c.Cin * c.k * c.k) ** 0.5
    w2 = torch.randn(c.cout2, c.Cin, 1, 1, generator=g, device=dev) / c.Cin ** 0.5 if c.cout2 else None
    bias = torch.randn(c.Cout, generator=g, device=dev) if c.bias else None
    bias2 = torch.randn(c.cout2, generator=g, device=dev) if (c.bias and c.cout2) else None
    wf, ldw = _pack_fwd(L, lib, c, w, w2, st)
    yb = torch.full((c.B, c.Ho, c.Wo, c.ldy), SENT, device=dev)
    nb = _nblk(lib, c)
    assert nb > 0
    part = torch.full((nb * 2 * c.Cout,), float("nan"), device=dev) if c.part else None
    p = [xb.data_ptr() + 4 * c.xoff, wf.data_ptr(), bias.data_ptr() if bias is not None else None, yb.data_ptr() + 4 * c.yoff,
         part.data_ptr() if part is not None else None]
    if c.cout2:
        y2b = torch.full((c.B, c.Ho, c.Wo, c.ldy2), SENT, device=dev)
        part2 = torch.full((nb * 2 * c.cout2,), float("nan"), device=dev) if c.part else None
        p += [bias2.data_ptr() if bias2 is not None else None, y2b.data_ptr() + 4 * c.y2off, part2.data_ptr() if part2 is not None else None]
    p += [None] * (10 - len(p)) + [tab.data_ptr() + 4 * c.xoff]
    _run1(L, _record(L, c.kind, _with_table(c.i or _fwd_slots(c, ldw), c.tld), p))
    torch.cuda.synchronize()
    x = xb[..., c.xoff:c.xoff + c.Cin]
    t = tab[:, c.xoff:c.xoff + c.Cin]
    errs = {}
    outs = [(yb, c.yoff, c.Cout, c.ldy, w, bias, part)] + ([(y2b, c.y2off, c.cout2, c.ldy2, w2, bias2, part2)] if c.cout2 else [])
    for n, (ybuf, off, co, ld, ww, bb, pp) in enumerate(outs):
        ref = conv_fwd64(x, ww, bb, c.s, t)
        errs[f"y{n}"] = rel_err(ybuf[..., off:off + co], ref)
        assert errs[f"y{n}"] < fwd_tol, (c.name(), errs)
        # the sentinel outside the output view survives
        assert bool((ybuf[..., :off] == SENT).all()) and bool((ybuf[..., off + co:] == SENT).all()), c.name()
        if pp is not None:
            errs[f"part{n}"] = part_err(pp, ref, co)
            assert errs[f"part{n}"] < part_tol, (c.name(), errs)
        del ref
    return errs


def run_wgrad(c: Case, seed: int, tol):
    L = _lib()
    lib = L.lib()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    xb = view_buf((c.B, c.H, c.W), c.ldx, c.xoff, c.Cin, g, dev)
    tab = make_table(c.Cin, c.tld, c.xoff, c.gate, c.sat, g, dev)
    dyb = view_buf((c.B, c.Ho, c.Wo), c.ldy, c.yoff, c.Cout, g, dev)
    nws = int(_ws_floats(lib, c))
    assert nws > 0
    ws = torch.full((nws,), float("nan"), device=dev)
    kk = c.k * c.k
    dw = torch.full((c.Cout * c.cin_real * kk,), float("nan"), device=dev)
    db = torch.full((c.Cout,), float("nan"), device=dev) if c.dbias else None
    p = [xb.data_ptr() + 4 * c.xoff, dyb.data_ptr() + 4 * c.yoff, dw.data_ptr(), ws.data_ptr(), db.data_ptr() if db is not None else None]
    p += [None] * 5 + [tab.data_ptr() + 4 * c.xoff]
    i = c.i or [c.ldx, c.ldy, c.B, c.H, c.W, c.Cin, c.cin_real, c.Cout, c.k, c.s]
    o = _record(L, c.kind, _with_table(i, c.tld), p, [nws])
    _run1(L, o)
    torch.cuda.synchronize()
    x, t, dy = xb[..., c.xoff:c.xoff + c.Cin], tab[:, c.xoff:c.xoff + c.Cin], dyb[..., c.yoff:c.yoff + c.Cout]
    ref = conv_wgrad64(x[..., :c.cin_real], dy, c.k, c.s, t[:, :c.cin_real])
    errs = {"dw": rel_err(dw.view(c.Cout, c.cin_real, c.k, c.k), ref)}
    assert errs["dw"] < tol, (c.name(), errs)
    if db is not None:
        dref = dy.double().reshape(-1, c.Cout).sum(0)
        errs["dbias"] = rel_err(db, dref)
        assert errs["dbias"] < FWD_TOL, (c.name(), errs)
    # a second run over a dirty workspace gives the same bits
    first = dw.clone(), (db.clone() if db is not None else None)
    ws.copy_(torch.randn(nws, generator=g, device=dev) * 1e3)
    dw.fill_(float("nan"))
    _run1(L, o)
    torch.cuda.synchronize()
    assert torch.equal(dw, first[0]), c.name()
    if db is not None:
        assert torch.equal(db, first[1]), c.name()
    return errs


# ---- section 2: reduced-size edge cases, one group per entry point ---------------------------------------------------------------

def _concat_gate(C):
    return tuple(int(c < C // 2) for c in range(C))


FWD_CASES = [
    # Winograd F(2x2, 3x3): odd tile counts (5 x 7), Cin = 48 (the m model), concat gates
    Case("OP_CONV_WINO_FWD", 2, 10, 14, 48, 32, ldx=56, xoff=4, ldy=44, yoff=8),
    Case("OP_CONV_WINO_FWD", 3, 6, 8, 64, 64, ldx=128, xoff=64, ldy=72, yoff=4, gate=_concat_gate(64)),
    Case("OP_CONV_WINO_FWD", 1, 18, 6, 32, 96, ldx=40, xoff=8, ldy=100, yoff=4, bias=True),
    # 3x3 stride 2, patch through LDS: odd H / W
    Case("OP_CONV_S2_FWD", 2, 9, 11, 32, 64, s=2, ldx=48, xoff=16, ldy=68, yoff=4),
    Case("OP_CONV_S2_FWD", 3, 7, 5, 64, 32, s=2, ldx=128, xoff=64, ldy=40, yoff=8, gate=_concat_gate(64)),
    # pointwise: the tiled and the streaming forms, ragged M, heads (bias, no partial sums, Cout 18 / 255)
    Case("OP_CONV_PW_FWD", 3, 9, 11, 64, 32, k=1, ldx=72, xoff=8, ldy=36, yoff=4),
    Case("OP_CONV_PW_FWD", 2, 13, 7, 128, 64, k=1, ldx=256, xoff=128, ldy=72, yoff=8, gate=_concat_gate(128)),
    Case("OP_CONV_PW_FWD", 1, 181, 191, 32, 32, k=1, ldx=64, xoff=32, ldy=40, yoff=4),
    Case("OP_CONV_PW_FWD", 2, 7, 9, 64, 18, k=1, ldx=68, xoff=4, ldy=24, yoff=4, bias=True, part=False),
    Case("OP_CONV_PW_FWD", 1, 5, 9, 128, 255, k=1, ldx=136, xoff=8, ldy=260, yoff=4, bias=True, part=False),
    # the sibling pair as one GEMM: even and uneven splits
    Case("OP_CONV_PW_FWD2", 2, 9, 13, 192, 64, k=1, cout2=128, ldx=200, xoff=8, ldy=68, yoff=4, ldy2=136, y2off=8),
    Case("OP_CONV_PW_FWD2", 3, 11, 7, 64, 32, k=1, cout2=32, ldx=128, xoff=64, ldy=36, yoff=4, ldy2=40, y2off=8,
         gate=_concat_gate(64)),
    Case("OP_CONV_PW_FWD2", 1, 150, 230, 32, 16, k=1, cout2=16, ldx=48, xoff=16, ldy=20, yoff=4, ldy2=24, y2off=4),
    # the narrow direct kernel (16-channel inputs)
    Case("OP_CONV_NARROW", 2, 9, 13, 16, 16, s=1, ldx=32, xoff=16, ldy=20, yoff=4),
    Case("OP_CONV_NARROW", 3, 11, 9, 16, 32, s=2, ldx=24, xoff=4, ldy=40, yoff=8, gate=_concat_gate(16)),
    # the gather GEMM: 2x2 / 4x4 maps, odd sizes, stride 2
    Case("OP_CONV_FWD", 8, 4, 4, 128, 128, ldx=256, xoff=128, ldy=132, yoff=4),
    Case("OP_CONV_FWD", 16, 2, 2, 64, 64, ldx=68, xoff=4, ldy=72, yoff=8, gate=_concat_gate(64)),
    Case("OP_CONV_FWD", 2, 5, 7, 48, 48, ldx=56, xoff=8, ldy=52, yoff=4),
    Case("OP_CONV_FWD", 2, 9, 11, 32, 64, s=2, ldx=40, xoff=4, ldy=68, yoff=4),
]

WGRAD_CASES = [
    Case("OP_CONV_WINO_BWD_WEIGHT", 2, 10, 14, 32, 64, ldx=40, xoff=8, ldy=68, yoff=4),
    Case("OP_CONV_WINO_BWD_WEIGHT", 3, 6, 8, 64, 32, ldx=128, xoff=64, ldy=36, yoff=4, gate=_concat_gate(64)),
    Case("OP_CONV_WINO_BWD_WEIGHT", 1, 12, 4, 32, 32, ldx=36, xoff=4, ldy=32),
    Case("OP_CONV_BWD_WEIGHT", 2, 9, 11, 48, 48, ldx=56, xoff=8, ldy=52, yoff=4),
    Case("OP_CONV_BWD_WEIGHT", 2, 9, 11, 64, 128, s=2, ldx=128, xoff=64, ldy=132, yoff=4, gate=_concat_gate(64)),
    Case("OP_CONV_BWD_WEIGHT", 8, 4, 4, 128, 128, ldx=132, xoff=4, ldy=128),
    Case("OP_CONV_BWD_WEIGHT", 16, 2, 2, 64, 64, ldx=72, xoff=8, ldy=68, yoff=4),
    Case("OP_CONV_PW_BWD_WEIGHT", 3, 9, 11, 64, 18, k=1, ldx=72, xoff=8, ldy=20),
    Case("OP_CONV_PW_BWD_WEIGHT", 2, 7, 9, 128, 255, k=1, ldx=136, xoff=4, ldy=256),
    Case("OP_CONV_PW_BWD_WEIGHT", 2, 13, 7, 128, 64, k=1, ldx=256, xoff=128, ldy=68, yoff=4, gate=_concat_gate(128)),
    Case("OP_CONV_PW_BWD_WEIGHT", 1, 97, 103, 32, 32, k=1, ldx=64, xoff=32, ldy=36, yoff=4),
    Case("OP_CONV_NARROW_BWD_WEIGHT", 2, 9, 13, 16, 16, s=1, ldx=32, xoff=16, ldy=20, yoff=4, dbias=True),
    Case("OP_CONV_NARROW_BWD_WEIGHT", 3, 11, 9, 16, 32, s=2, ldx=24, xoff=4, ldy=36, yoff=4, dbias=True, gate=_concat_gate(16)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c.name())
def test_prologue_forward_edges(c, record_property):
    record_property("errors", run_forward(c, seed=_seed(c.name())))


@pytest.mark.gpu
@pytest.mark.parametrize("c", WGRAD_CASES, ids=lambda c: c.name())
def test_prologue_weight_gradient_edges(c, record_property):
    record_property("errors", run_wgrad(c, seed=_seed(c.name()), tol=PW_WGRAD_TOL if c.kind == "OP_CONV_PW_BWD_WEIGHT" else WGRAD_TOL))


def test_edge_cases_are_on_their_kernels():
    """Every reduced case is a shape its family's gate accepts, so the GPU tests above run the kernel they name (host queries)."""
    lib = _lib().lib()
    for c in FWD_CASES + WGRAD_CASES:
        M = c.B * c.H * c.W
        if c.kind == "OP_CONV_WINO_FWD":
            assert lib.yh_conv_wino_blocks(c.B, c.H, c.W) > 0 and c.Cin % 16 == 0, c.name()
        elif c.kind == "OP_CONV_S2_FWD":
            assert lib.yh_conv_s2_ok(c.B, c.H, c.W, c.Cin, c.Cout) == 1, c.name()
        elif c.kind in ("OP_CONV_PW_FWD", "OP_CONV_PW_FWD2"):
            assert lib.yh_conv_pw_prologue_ok(M, c.Cin, c.Cout + c.cout2) == 1, c.name()
        elif c.kind == "OP_CONV_NARROW":
            assert lib.yh_conv_narrow_ok(c.Cin, c.Cout, 3, c.s) == 1, c.name()
        elif c.kind == "OP_CONV_BWD_WEIGHT":
            assert lib.yh_conv_bwd_weight_prologue_ok(c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.s) == 1, c.name()
        elif c.kind == "OP_CONV_NARROW_BWD_WEIGHT":
            assert lib.yh_conv_narrow_bwd_weight_ok(c.Cin, c.cin_real, c.Cout, 3, c.s) == 1, c.name()
        elif c.kind == "OP_CONV_WINO_BWD_WEIGHT":
            assert lib.yh_conv_wino_bwd_weight_ws(c.B, c.H, c.W, c.Cin, c.Cout) > 0 and c.ldx % 4 == 0 and c.ldy % 4 == 0, c.name()
        assert c.xoff % 4 == 0 and c.ldx >= c.xoff + c.Cin and c.ldy >= c.yoff + c.Cout
        assert c.tld >= c.xoff + c.Cin and c.tld % 4 == 0
    kinds = {c.kind for c in FWD_CASES + WGRAD_CASES}
    assert kinds == set(ACT_KINDS)


# ---- yh_bn_silu_fwd_res: the residual reader -------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ResCase:
    B: int
    H: int
    W: int
    C: int
    ldy: int
    ldr: int
    roff: int
    ldo: int
    ooff: int
    up: int = 0
    tld: int = 0
    gate: Tuple[int, ...] = ()
    sat: int = 1

    def name(self):
        return f"{self.B}x{self.H}x{self.W}-C{self.C}-ldr{self.ldr}o{self.roff}-ldo{self.ldo}o{self.ooff}-up{self.up}"


def run_silu_res(c: ResCase, seed: int, i=None):
    L = _lib()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    C, M = c.C, c.B * c.H * c.W
    tld = c.tld or rup4(c.ldr) + 4
    gate = c.gate or tuple(int(k % 3 != 0) for k in range(C))
    y = view_buf((c.B, c.H, c.W), c.ldy, 0, C, g, dev)
    rb = view_buf((c.B, c.H, c.W), c.ldr, c.roff, C, g, dev)
    rtab = make_table(C, tld, c.roff, gate, c.sat, g, dev)
    coef = torch.full((4 * C,), float("nan"), device=dev)
    coef[:C] = torch.rand(C, generator=g, device=dev) + 0.5
    coef[C:2 * C] = torch.randn(C, generator=g, device=dev)
    f = 2 if c.up else 1
    ob = torch.full((c.B, c.H * f, c.W * f, c.ldo), SENT, device=dev)
    p = [y.data_ptr(), coef.data_ptr(), rb.data_ptr() + 4 * c.roff, ob.data_ptr() + 4 * c.ooff, rtab.data_ptr() + 4 * c.roff]
    i = list(i) if i else [c.ldy, c.ldr, c.ldo, C, c.H, c.W, c.up, tld]
    _run1(L, _record(L, "OP_BN_SILU_FWD", i, p, [M]))
    torch.cuda.synchronize()
    z = y[..., :C].double() * coef[:C].double() + coef[C:2 * C].double()
    ref = z * torch.sigmoid(z) + prologue64(rb[..., c.roff:c.roff + C], rtab[:, c.roff:c.roff + C])
    if c.up:
        ref = ref.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    err = rel_err(ob[..., c.ooff:c.ooff + C], ref)
    assert err < FWD_TOL, (c.name(), err)
    assert bool((ob[..., :c.ooff] == SENT).all()) and bool((ob[..., c.ooff + C:] == SENT).all()), c.name()
    return {"out": err}


RES_CASES = [ResCase(2, 7, 9, 32, 32, 64, 32, 72, 8), ResCase(3, 5, 6, 64, 68, 128, 64, 64, 0, gate=_concat_gate(64)),
             ResCase(2, 4, 5, 16, 20, 24, 4, 32, 16, up=1), ResCase(1, 3, 7, 48, 48, 56, 8, 52, 4, up=1, gate=_concat_gate(48))]


@pytest.mark.gpu
@pytest.mark.parametrize("c", RES_CASES, ids=lambda c: c.name())
def test_bn_silu_residual_prologue(c, record_property):
    record_property("errors", run_silu_res(c, seed=_seed(c.name())))


# ---- yh_bn_finalize_x: the table writer --------------------------------------------------------------------------------------------

def run_finalize(nblk, C, M, toff, tld, track=True, acc=True, seed=0):
    """yh_bn_finalize_x through a one-record list against yh_bn_finalize on the same partials: coef, running statistics and
    num_batches_tracked bitwise equal; xscale / xshift bitwise equal to coef's scale / shift; the gate row and the table columns
    outside the view untouched; the backward accumulators zeroed; scale / shift against fp64."""
    L = _lib()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    mean = torch.randn(C, generator=g, device=dev, dtype=torch.float64) * 0.5
    var = torch.rand(C, generator=g, device=dev, dtype=torch.float64) * 2 + 0.25
    wts = torch.rand(nblk, C, generator=g, device=dev, dtype=torch.float64) + 0.1
    wts /= wts.sum(0)
    part = torch.stack([wts * (M * mean), wts * (M * (var + mean * mean))], 1).float().contiguous()     # [nblk][2][C]
    gamma = torch.rand(C, generator=g, device=dev) + 0.5
    beta = torch.randn(C, generator=g, device=dev)
    rm0, rv0 = torch.randn(C, generator=g, device=dev), torch.rand(C, generator=g, device=dev) + 0.5
    tab = torch.full((3, tld), float("nan"), device=dev)
    tab[2, toff:toff + C] = torch.tensor([float(k % 3 != 0) for k in range(C)], device=dev)
    tab0 = tab.clone()
    bacc = torch.randint(-2 ** 40, 2 ** 40, (2 * C,), generator=g, device=dev, dtype=torch.int64)
    rm, rv, nbt = rm0.clone(), rv0.clone(), torch.tensor([5], device=dev, dtype=torch.int64)
    coef = torch.full((4 * C,), float("nan"), device=dev)
    mom, eps = 0.03, 1e-3
    p = [part.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr() if track else None, rv.data_ptr() if track else None,
         coef.data_ptr(), nbt.data_ptr() if track else None, tab.data_ptr() + 4 * toff, tab.data_ptr() + 4 * (tld + toff),
         bacc.data_ptr() if acc else None]
    o = _record(L, "OP_BN_FINALIZE", [nblk, C], p, [M])
    o.f[0], o.f[1] = mom, eps
    _run1(L, o)
    rm2, rv2, nbt2 = rm0.clone(), rv0.clone(), torch.tensor([5], device=dev, dtype=torch.int64)
    coef2 = torch.full((4 * C,), float("nan"), device=dev)
    L.check(lib.yh_bn_finalize(part.data_ptr(), nblk, M, gamma.data_ptr(), beta.data_ptr(), rm2.data_ptr() if track else None,
                               rv2.data_ptr() if track else None, mom, eps, coef2.data_ptr(), C, nbt2.data_ptr() if track else None, st))
    torch.cuda.synchronize()
    assert torch.equal(coef, coef2)
    assert torch.equal(rm, rm2) and torch.equal(rv, rv2) and torch.equal(nbt, nbt2)
    if track:
        assert int(nbt) == 6
    assert torch.equal(tab[0, toff:toff + C], coef[:C]) and torch.equal(tab[1, toff:toff + C], coef[C:2 * C])
    keep = torch.ones(3, tld, dtype=torch.bool, device=dev)
    keep[:2, toff:toff + C] = False
    assert torch.equal(tab[keep].isnan(), tab0[keep].isnan()) and torch.equal(tab[keep].nan_to_num(), tab0[keep].nan_to_num())
    if acc:
        assert bool((bacc == 0).all())
    s = part.double().sum(0)
    mu = s[0] / M
    sc = gamma.double() / torch.sqrt(s[1] / M - mu * mu + eps)
    err = max(rel_err(coef[:C], sc), rel_err(coef[C:2 * C], beta.double() - mu * sc))
    assert err < FWD_TOL, err
    return {"coef": err}


@pytest.mark.gpu
@pytest.mark.parametrize("nblk,C,M,toff,tld,track,acc", [(37, 64, 37 * 256 + 5, 4, 132, True, True), (1, 16, 99, 0, 20, True, True),
                                                          (300, 128, 10 ** 6, 64, 196, False, True), (5, 48, 4000, 8, 60, True, False)])
def test_bn_finalize_writes_consumer_table(nblk, C, M, toff, tld, track, acc, record_property):
    record_property("errors", run_finalize(nblk, C, M, toff, tld, track, acc, seed=nblk + C))


# ---- launcher contracts the planner relies on (argument checks only: none of these launches a kernel) -----------------------------

def _rejects(L, rc, sentinel):
    torch.cuda.synchronize()
    assert rc != 0
    assert L.lib().yh_last_error().decode()
    assert bool((sentinel == SENT).all())


@pytest.mark.gpu
def test_prologue_contracts():
    L = _lib()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    B, H, W, Cin, Cout = 2, 8, 8, 32, 32
    M = B * H * W
    x = torch.randn(B, H, W, Cin, device=dev)
    dy = torch.randn(B, H, W, Cout, device=dev)
    tab = torch.zeros(3, 2 * Cin + 8, device=dev)
    tab[0] = 1.0
    T, tld = tab.data_ptr(), tab.shape[1]
    Tm = T + 4                                     # 4-byte aligned, not 16
    y = torch.full((B, H, W, Cout), SENT, device=dev)
    wbig = torch.zeros(16 * Cin * Cout * 4, device=dev)      # large enough for every family's pack
    part = torch.zeros(4096 * 2 * Cout, device=dev)
    ws = torch.zeros(1 << 22, device=dev)
    dw = torch.full((Cout * Cin * 9,), SENT, device=dev)
    xp, yp, wp, pp, dp, wsp, dyp = x.data_ptr(), y.data_ptr(), wbig.data_ptr(), part.data_ptr(), dw.data_ptr(), ws.data_ptr(), dy.data_ptr()
    nws = ws.numel()
    # tables that are not 16-byte aligned, and strides below Cin
    for t, ld in ((Tm, tld), (T, Cin - 4)):
        _rejects(L, lib.yh_conv_wino_fwd_act(xp, Cin, t, ld, wp, Cout, None, yp, Cout, None, B, H, W, Cin, Cout, st), y)
        _rejects(L, lib.yh_conv_s2_fwd_act(xp, Cin, t, ld, wp, Cout, None, yp, Cout, None, B, H, W, Cin, Cout, st), y)
        _rejects(L, lib.yh_conv_fwd_act(xp, Cin, t, ld, wp, Cout, None, yp, Cout, None, B, H, W, Cin, Cout, 3, 1, st), y)
        _rejects(L, lib.yh_conv_pw_fwd_act(xp, Cin, t, ld, wp, Cout, None, yp, Cout, None, M, Cin, Cout, st), y)
        _rejects(L, lib.yh_conv_pw_fwd2_act(xp, Cin, t, ld, wp, Cout, None, yp, 16, None, 16, None, yp + 64, 16, None, 16, M, Cin, st), y)
        _rejects(L, lib.yh_conv_wino_bwd_weight_act(xp, Cin, t, ld, dyp, Cout, dp, wsp, nws, B, H, W, Cin, Cout, st), dw)
        _rejects(L, lib.yh_conv_bwd_weight_act(xp, Cin, t, ld, dyp, Cout, dp, wsp, nws, B, H, W, Cin, Cin, Cout, 3, 1, st), dw)
        x16, t16 = x[..., :16].contiguous(), (t if ld == tld else T)
        _rejects(L, lib.yh_conv_narrow_act(x16.data_ptr(), 16, t16, ld if ld == tld else 12, wp, 32, None, yp, Cout, None, B, H, W, 16, 16,
                                           1, st), y)
        _rejects(L, lib.yh_conv_narrow_bwd_weight_act(x16.data_ptr(), 16, t16, ld if ld == tld else 12, dyp, Cout, dp, None, wsp, nws, B, H,
                                                      W, 16, 16, 16, 1, st), dw)
    _rejects(L, lib.yh_conv_pw_bwd_weight_act(xp, Cin, T, Cin - 4, dyp, Cout, dp, wsp, nws, M, Cin, Cout, st), dw)
    # cin_real != Cin on the gather weight gradient
    assert lib.yh_conv_bwd_weight_prologue_ok(B, H, W, Cin, Cout, 3, 1) == 1
    _rejects(L, lib.yh_conv_bwd_weight_act(xp, Cin, T, tld, dyp, Cout, dp, wsp, nws, B, H, W, Cin, Cin - 4, Cout, 3, 1, st), dw)
    # the narrow forward with a table needs a 16-channel input
    x4 = torch.randn(B, 2 * H, 2 * W, 4, device=dev)
    assert lib.yh_conv_narrow_ok(4, 16, 3, 2) == 1
    _rejects(L, lib.yh_conv_narrow_act(x4.data_ptr(), 4, T, tld, wp, 16, None, yp, Cout, None, B, 2 * H, 2 * W, 4, 16, 2, st), y)
    # a pointwise shape on the register-direct GEMM, which has no prologue
    shapes = [(m, ci, co) for m in (96, 200, 1000) for ci in (8, 16, 24, 40) for co in (8, 16, 32) if not lib.yh_conv_pw_prologue_ok(m, ci, co)]
    assert shapes
    m, ci, co = shapes[0]
    xs, ys = torch.randn(m, ci, device=dev), torch.full((m, co), SENT, device=dev)
    _rejects(L, lib.yh_conv_pw_fwd_act(xs.data_ptr(), ci, T, tld, wp, rup4(co), None, ys.data_ptr(), co, None, m, ci, co, st), ys)
    # Winograd weight gradient: a dY row stride that is even but not a multiple of 4 routes to the register kernel (no prologue)
    dy34 = torch.randn(B, H, W, 34, device=dev)
    _rejects(L, lib.yh_conv_wino_bwd_weight_act(xp, Cin, T, tld, dy34.data_ptr(), 34, dp, wsp, nws, B, H, W, Cin, Cout, st), dw)
    assert lib.yh_conv_wino_bwd_weight(xp, Cin, dy34.data_ptr(), 34, dp, wsp, nws, B, H, W, Cin, Cout, st) == 0   # fine without one
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("flip,acc", [(1, 0), (0, 1), (1, 1)])
def test_narrow_record_with_table_refuses_flip_or_accumulate(flip, acc):
    """A CONV_NARROW record carrying a prologue table may not also ask for flipped taps or accumulation: yh_conv_narrow_act has
    neither, so the dispatcher refuses the record instead of dropping them."""
    L = _lib()
    dev = torch.device("cuda")
    B, H, W = 2, 6, 6
    x = torch.randn(B, H, W, 16, device=dev)
    tab = torch.zeros(3, 20, device=dev)
    w = torch.zeros(9 * 16 * 16, device=dev)
    y = torch.full((B, H, W, 16), SENT, device=dev)
    o = _record(L, "OP_CONV_NARROW", _with_table([16, 16, 16, B, H, W, 16, 16, 1, flip, acc], 20),
                [x.data_ptr(), w.data_ptr(), None, y.data_ptr(), None] + [None] * 5 + [tab.data_ptr()])
    with pytest.raises(RuntimeError, match="CONV_NARROW record with an input prologue table"):
        _run1(L, o)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


# ---- section 3: the plan-driven sweep at the real shapes ---------------------------------------------------------------------------

SWEEP_PLANS = [("headline", 1, "s", 640, 64), ("nc80", 80, "s", 320, 7), ("64px", 1, "s", 64, 64), ("m256", 1, "m", 256, 4)]
_SIZES = {"n": (0.25, 0.33), "s": (0.50, 0.33), "m": (0.75, 0.67), "l": (1.0, 1.0), "x": (1.25, 1.33)}


def _compile_cpu_plan(nc, size, img, batch):
    from yolo_from_scratch_amd import graph as G, modules as Mo
    torch.manual_seed(0)
    wm, dm = _SIZES[size]
    m = Mo.YOLO(num_classes=nc, img_size=img, width_mult=wm, depth_mult=dm).train(True)
    plan = G.Plan(torch.device("cpu"), (batch, 3, img, img), True, False, "f32")
    m._trace(plan)
    plan.compile(m._grad_views(torch.device("cpu")))
    return plan


def _locate(plan, addr, ld):
    """Channel offset of a view at `addr` with row stride `ld` inside its plan buffer (0 for a layer's own tensor)."""
    for b in plan.buffers:
        for t in (b.data, b._grad):
            if t is not None and t.data_ptr() <= addr < t.data_ptr() + t.numel() * t.element_size():
                e = (addr - t.data_ptr()) // t.element_size()
                assert t.shape[-1] == ld
                return e % ld
    return 0


def _table_of(plan, tp):
    for b in plan.buffers:
        t = b._icoef
        if t is not None and t.data_ptr() <= tp < t.data_ptr() + t.numel() * 4:
            return (tp - t.data_ptr()) // 4
    raise AssertionError("prologue table outside every plan buffer")


def _gate_row(tp, tld, C):
    return tuple(int(v != 0) for v in np.frombuffer(ctypes.string_at(tp + 8 * tld, 4 * C), dtype=np.float32))


def enumerate_plan(plan):
    """Every op record of a CPU-compiled plan that reads or writes a prologue table, as (kind, signature) with the record's
    shapes, ld's, offsets, the real gate row and the 16-byte alignment of the table pointer."""
    import yolo_from_scratch_amd._lib as L
    names = {getattr(L, k): k for k in ACT_KINDS + ("OP_BN_FINALIZE", "OP_BN_SILU_FWD")}
    out = []
    for lst in (plan.fwd_ops, plan.bwd_ops):
        arr, n = lst
        for j in range(n):
            o = arr[j]
            kind = names.get(o.kind)
            i = tuple(o.i)
            if kind in ACT_KINDS and o.p[10]:
                toff = _table_of(plan, o.p[10])
                if kind in WGRAD_KINDS:
                    ldx, lddy, B, H, W, cin, creal, cout, k, s = i[:10]
                    if kind == "OP_CONV_NARROW_BWD_WEIGHT":
                        k = 3
                    xoff = _locate(plan, o.p[0], ldx)
                    c = Case(kind, B, H, W, cin, cout, k=k, s=s, cin_real=creal, ldx=ldx, xoff=xoff, tld=i[17], ldy=lddy,
                             yoff=_locate(plan, o.p[1], lddy), dbias=bool(o.p[4]), gate=_gate_row(o.p[10], i[17], cin), i=i)
                else:
                    ldx, ldw, ldy, B, H, W, cin, cout = i[:8]
                    k, s = (3, i[8]) if kind == "OP_CONV_NARROW" else (1, 1) if kind == "OP_CONV_PW_FWD2" else i[8:10]
                    extra = dict(cout2=i[9], ldy2=i[8], y2off=_locate(plan, o.p[6], i[8])) if kind == "OP_CONV_PW_FWD2" else {}
                    c = Case(kind, B, H, W, cin, cout, k=k, s=s, ldx=ldx, xoff=_locate(plan, o.p[0], ldx), tld=i[17], ldy=ldy,
                             yoff=_locate(plan, o.p[3], ldy), bias=bool(o.p[2]), part=bool(o.p[4]), gate=_gate_row(o.p[10], i[17], cin),
                             i=i, **extra)
                assert toff == c.xoff
                out.append((kind, c, o.p[10] % 16 == 0))
            elif kind == "OP_BN_SILU_FWD" and o.p[4]:
                ldy, ldr, ldo, C, H, W, up, rld = i[:8]
                M = o.l[0]
                rc = ResCase(M // (H * W), H, W, C, ldy, ldr, _locate(plan, o.p[2], ldr), ldo, _locate(plan, o.p[3], ldo), up, rld,
                             _gate_row(o.p[4], rld, C))
                assert _table_of(plan, o.p[4]) == rc.roff
                out.append((kind, (rc, i), o.p[4] % 16 == 0))
            elif kind == "OP_BN_FINALIZE" and o.p[7]:
                toff = _table_of(plan, o.p[7])
                tld = (o.p[8] - o.p[7]) // 4
                sig = (i[0], i[1], o.l[0], toff, tld, bool(o.p[3]), bool(o.p[9]))
                out.append((kind, sig, o.p[7] % 16 == 0 and o.p[8] % 16 == 0))
    return out


def _sweep():
    """Distinct launch signatures over the four plans, in plan order (first plan that has a signature names it)."""
    seen, cases = set(), []
    for label, nc, size, img, batch in SWEEP_PLANS:
        for kind, c, _ in enumerate_plan(_compile_cpu_plan(nc, size, img, batch)):
            key = (kind, c)
            if key in seen:
                continue
            seen.add(key)
            if kind == "OP_BN_SILU_FWD":
                nm = "bn_silu_fwd-" + c[0].name()
            elif kind == "OP_BN_FINALIZE":
                nm = "bn_finalize-nblk{}-C{}-M{}-toff{}-tld{}-track{}-acc{}".format(*c)
            else:
                nm = c.name()
            cases.append(pytest.param(kind, c, id=f"{label}-{nm}-{len(cases)}"))
    return cases


try:
    SWEEP = _sweep()
except Exception as e:         # a library that is not built or a planner that fails: one failing case says so
    SWEEP = [pytest.param("ERROR", repr(e), id="sweep-enumeration-failed")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,c", SWEEP)
def test_prologue_plan_sweep(kind, c, record_property):
    assert kind != "ERROR", c
    seed = _seed(str(c))
    if kind == "OP_BN_SILU_FWD":
        errs = run_silu_res(c[0], seed, i=c[1])
    elif kind == "OP_BN_FINALIZE":
        errs = run_finalize(*c, seed=seed)
    elif kind in WGRAD_KINDS:
        errs = run_wgrad(c, seed, WGRAD_TOL)
    else:
        errs = run_forward(c, seed)
    record_property("errors", errs)             # the measured errors, in the junit report
    torch.cuda.empty_cache()


def test_sweep_enumeration_guard():
    """CPU guard for the sweep: the headline plan still has prologue launches of every `_act` kind, more than 100 of them, at least
    one table writer and one residual reader, and every table pointer is 16-byte aligned.  Lower bounds, not exact counts."""
    recs = enumerate_plan(_compile_cpu_plan(1, "s", 640, 64))
    kinds = [k for k, _, _ in recs]
    assert set(ACT_KINDS) <= set(kinds)
    assert sum(k in ACT_KINDS for k in kinds) > 100
    assert kinds.count("OP_BN_FINALIZE") >= 1 and kinds.count("OP_BN_SILU_FWD") >= 1
    assert all(al for _, _, al in recs)
    assert len(SWEEP) > 150 and all(p.values[0] != "ERROR" for p in SWEEP)
