"""Canonical dump of the op lists the planner emits, for a before/after comparison of a planner refactor.

Runs on the CPU: plans are traced and compiled on torch.device("cpu") (the library's sizing queries are host code), nothing is
launched.  Every address in the op records and in the descriptor tables of the *_MULTI ops is replaced by the ordinal of its
first appearance, so two dumps are equal exactly when the two planners emit the same ops, in the same order, with the same
integer / float arguments and the same aliasing between pointers.

usage: python plan_dump.py REPO OUT.txt     (REPO: the checkout whose planner is dumped)"""
import ctypes, os, struct, sys

repo, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, repo)
import torch
from yolo_from_scratch_amd import _lib as L, graph as G, modules as Mo

TABLES = {"OP_PACK_WEIGHTS_MULTI": "<QQQiiiiiiii", "OP_BF16_PACK_MULTI": "<QQQiiiiiiii", "OP_WINO_WEIGHTS_MULTI": "<QQiiii",
          "OP_LAT_PACK_MULTI": "<QQiiii", "OP_PW_PACK_MULTI": "<QQQiiiiii", "OP_FOLD_OIHW_MULTI": "<QQQQQQQQiifi"}
TABLES = {getattr(L, k): v for k, v in TABLES.items()}
NAMES = {v: k for k, v in vars(L).items() if k.startswith("OP_") and isinstance(v, int)}
DEV = torch.device("cpu")

# (label, env, nc, size, img, batch, training, dtype, need_input_grad)
CASES = [("train f32 headline", {}, 1, "s", 640, 64, True, "f32", False),
         ("train f32 nc80 ragged", {}, 80, "s", 320, 7, True, "f32", False),
         ("train f32 input grad", {}, 3, "s", 256, 4, True, "f32", True),
         ("train f32 64px bs64", {}, 1, "s", 64, 64, True, "f32", False),
         ("train f32 generic", {"YH_GENERIC": "1"}, 1, "s", 320, 8, True, "f32", False),
         ("train f32 unfused", {"YH_FUSE_ACT": "0"}, 1, "s", 320, 8, True, "f32", False),
         ("train bf16 nc80", {}, 80, "s", 640, 16, True, "bf16", False),
         ("train bf16 input grad", {}, 3, "s", 256, 4, True, "bf16", True),
         ("eval bs1", {}, 1, "s", 640, 1, False, "f32", False),
         ("eval bs1 nc80", {}, 80, "s", 640, 1, False, "f32", False),
         ("eval bs32", {}, 1, "s", 640, 32, False, "f32", False),
         ("eval slow", {"YH_EVAL_FAST": "0"}, 1, "s", 640, 8, False, "f32", False)]
for sz in ("n", "m", "l", "x"):
    CASES += [(f"train f32 {sz}", {}, 1, sz, 256, 4, True, "f32", False), (f"eval {sz}", {}, 1, sz, 256, 4, False, "f32", False)]
SIZES = {"n": (0.25, 0.33), "s": (0.50, 0.33), "m": (0.75, 0.67), "l": (1.0, 1.0), "x": (1.25, 1.33)}


def dump(plan, w):
    ids = {0: 0}

    def canon(a):
        return ids.setdefault(a, len(ids)) if a else 0
    for name in ("prep_ops", "fwd_ops", "bwd_ops"):
        lst = getattr(plan, name)
        if lst is None:
            continue
        arr, n = lst
        w(f"  {name} {n}")
        for k in range(n):
            o = arr[k]
            w(f"    {NAMES.get(o.kind, o.kind)} lane={o.lane} i={list(o.i)} f={[round(x, 9) for x in o.f]} l={list(o.l)} "
              f"p={[canon(x or 0) for x in o.p]}")
            fmt = TABLES.get(o.kind)
            if fmt:
                sz = struct.calcsize(fmt)
                raw = ctypes.string_at(o.p[0], sz * o.i[0])
                for row in struct.iter_unpack(fmt, raw):
                    w("      " + str([canon(v) if c == "Q" else v for c, v in zip(fmt[1:], row)]))


with open(out, "w") as fh:
    w = lambda s: fh.write(s + "\n")
    for label, env, nc, sz, img, bs, training, dtype, need_dx in CASES:
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            torch.manual_seed(0)
            wm, dm = SIZES[sz]
            m = Mo.YOLO(num_classes=nc, img_size=img, width_mult=wm, depth_mult=dm).train(training)
            plan = G.Plan(DEV, (bs, 3, img, img), training, need_dx, dtype)
            m._trace(plan)
            plan.compile(m._grad_views(DEV) if training else None)
            w(f"== {label}")
            dump(plan, w)
        except Exception as e:          # a planner that fails on a case is a finding, not a crash of the dump
            w(f"== {label}\n  ERROR {type(e).__name__}: {e}")
        finally:
            for k, v in saved.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
