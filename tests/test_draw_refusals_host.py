"""The eighteen draw entry points side by side on host-only contexts: one fixed list of arguments per entry point, every one refused -- or, the empty
cases, accepted -- before anything touches a device, and the whole transcript (entry point, case, code, and each message with the slot it was stored in)
held to tests/golden/draw_refusals.txt.  That file was written by the library of the commit BEFORE the host's draw paths were brought down to one
description of a draw's surfaces (its first line names the commit); it is never written by the code under test:

    tools/ab_build_commit.sh pre <commit>
    ATMO_HIP_LIB=godot_atmosphere_shader_amd/libatmo_hip_pre.so PYTHONPATH=. python tests/test_draw_refusals_host.py <commit>

Pointers are small fixed integers that no refusal dereferences, so no address appears in a message.  Not listed, because a host-only context would go on
to a device call: any well-formed draw with a tile, and the unsupported modes for the entry points that draw in every mode (atmo_render, _composite,
_tiles, _tiles_split, and an RGBA32F atmo_render_target)."""
import ctypes as C
import os

import numpy as np

from test_views_proxy_host import AWAY, FAR, ROOT, SIZE, _frame, _host_ctx, _mat

GOLDEN = os.path.join(ROOT, "tests", "golden", "draw_refusals.txt")
F32, F16, U8, SRGB8 = 0, 1, 2, 16          # AtmoTargetFormat
D32, D16 = 0, 1                            # AtmoDepthFormat
DEPTH, RGBA, IMG, TEX, TILES, STEP = 0x1000, 0x2000, 0x100000, 0x800000, 0x3000, 0x10000
W, H = FAR.width, FAR.height               # 64 x 36
EMPTY = (5, 5, 5, 30)

SINGLE = ("atmo_render", "atmo_render_composite", "atmo_render_tiles", "atmo_render_tiles_split", "atmo_render_target", "atmo_render_depth_target")
PROXY = ("atmo_render_proxy", "atmo_render_proxy_composite", "atmo_render_proxy_target", "atmo_render_proxy_depth_target")
VIEWS = ("atmo_render_views", "atmo_render_views_target", "atmo_render_views_depth_target", "atmo_render_views_proxy", "atmo_render_views_proxy_target",
         "atmo_render_views_proxy_depth_target")
PLANETS = ("atmo_render_planets", "atmo_plan_planets")
ENTRY_POINTS = SINGLE + PROXY + VIEWS + PLANETS
MODES = ("precision 0", "precision 2", "64 view steps", "lane split 2")


def _has(entry, word):
    return word in entry.replace("atmo_render_", "").replace("atmo_plan_", "").split("_") or (word == "target" and entry in PLANETS)


def _cases(entry):
    """[(name, overrides)]: in a batch, the per-draw overrides go to view / draw 1 of two."""
    batch, proxy = entry in VIEWS + PLANETS, _has(entry, "proxy") or entry in PLANETS
    target, depth_source, tiles = _has(entry, "target"), _has(entry, "depth"), _has(entry, "tiles")
    c = [("null ctx", dict(ctx=None))]
    if entry in VIEWS:
        c += [("null views", dict(null_list=True)), ("n_views -1", dict(n=-1)), ("n_views 9", dict(n=9)), ("n_views 0, null views", dict(n=0, null_list=True))]
    elif entry in PLANETS:
        c += [("null draws", dict(null_list=True)), ("n_draws -1", dict(n=-1)), ("n_draws 65", dict(n=65)), ("n_draws 0, null draws", dict(n=0, null_list=True)),
              ("null ctx in draw 1", dict(draw_ctx=None))]
    else:
        c += [("null frame", dict(null_frame=True))]
    c += [("viewport 65537", dict(vw=65537)), ("viewport 0", dict(vw=0)), ("inverted rect", dict(rect=(10, 0, 5, H))), ("rect beyond the viewport", dict(rect=(0, 0, W + 1, H)))]
    if tiles:
        c += [("n_tiles -1", dict(n_tiles=-1)), ("null tile list", dict(tiles=None)), ("n_tiles 0", dict(n_tiles=0, null_frame=True))]
    if entry == "atmo_render_tiles_split":
        c += [("n_heavy -1", dict(n_heavy=-1)), ("n_heavy beyond n_tiles", dict(n_heavy=5))]
    if proxy:
        c += [("null model matrix", dict(model=None)), ("box_size 0", dict(size=0.0)), ("box_size infinite", dict(size=float("inf"))),
              ("box_size nan", dict(size=float("nan"))), ("singular model matrix", dict(model=np.zeros((4, 4))))]
    if target:
        c += [("unknown target format", dict(fmt=3)), ("null target pixels", dict(pixels=None)), ("misaligned target pixels", dict(fmt=F16, pixels=IMG + 4)),
              ("pitch too small", dict(fmt=U8, pitch=(W - 1) * 4, composite=1)), ("pitch no multiple of the pixel", dict(fmt=U8, pitch=W * 4 + 2))]
        if not batch:
            c += [("null target", dict(null_target=True))]
    else:
        c += [("null rgba", dict(rgba=None)), ("misaligned rgba", dict(rgba=RGBA + 8))]
    if depth_source:
        c += [("unknown depth format", dict(dfmt=7)), ("null depth texels", dict(texels=None)), ("misaligned depth texels", dict(texels=TEX + 2)),
              ("depth pitch too small", dict(dpitch=W * 4 - 4)), ("depth pitch no multiple of the texel", dict(dfmt=D16, dpitch=W * 2 + 1))]
        if not batch:
            c += [("null depth", dict(null_depth=True))]
    else:
        c += [("null depth", dict(depth=None))]
    if entry in VIEWS:   # (the planets call takes both: it orders what overlaps, and a format is a launch key)
        c += [("mixed formats", dict(fmt=U8))] if target else []
        c += [("overlapping outputs", dict(rgba=RGBA, pixels=IMG))]
    if proxy or entry in VIEWS or (target and entry != "atmo_render_target") or depth_source:
        c += [(m, dict(mode=m)) for m in MODES]
    elif entry == "atmo_render_target":
        c += [(m + ", RGBA16F", dict(mode=m, fmt=F16)) for m in MODES]
    # accepted: nothing to draw
    if entry in SINGLE:
        c += [("empty rect, null pointers", dict(rect=EMPTY, depth=None, rgba=None, null_depth=True))]
    if entry in PROXY:
        c += [("empty rect", dict(rect=EMPTY)), ("empty rect, null depth", dict(rect=EMPTY, depth=None, null_depth=True)), ("box behind the camera", dict(cam=AWAY))]
    if entry == "atmo_render_proxy_target":
        c += [("empty RGBA32F row, null model matrix", dict(rect=EMPTY, fmt=F32, model=None)), ("empty RGBA32F row, pitch given, null model matrix",
                                                                                               dict(rect=EMPTY, fmt=F32, pitch=64, model=None))]
    if batch:
        c += [("every rect empty, null pointers", dict(every=dict(rect=EMPTY, depth=None, rgba=None, texels=None)))]
        if proxy:
            c += [("every box behind the camera", dict(every=dict(cam=AWAY)))]
    if entry in VIEWS and proxy:
        c += [("n_views 0, null model matrix", dict(n=0, model=None))]
    return c


class _Lib:
    def __init__(self):
        from godot_atmosphere_shader_amd import _native as N

        self.N, self.lib = N, N.load()
        direct = dict(light_mode=N.LIGHT_DIRECT, light_steps=8)     # the direct-light atmosphere: no texture to miss
        self.a, self.b = _host_ctx(N.VARIANT_NO_CLOUDS, **direct), _host_ctx(N.VARIANT_NO_CLOUDS, **direct)
        # (precision 0 is another form of the cloud kernels only; a cloud context without its textures is refused for those where they are checked first)
        self.odd = {m: _host_ctx(N.VARIANT_CLOUDS_HIGH if m == "precision 0" else N.VARIANT_NO_CLOUDS, view_steps=64 if m == "64 view steps" else 0, **direct)
                    for m in MODES}
        assert self.lib.atmo_set_precision(self.odd["precision 0"], 0) == N.ATMO_OK and self.lib.atmo_set_precision(self.odd["precision 2"], 2) == N.ATMO_OK
        assert self.lib.atmo_set_lane_split(self.odd["lane split 2"], 2) == N.ATMO_OK

    def close(self):
        for ctx in [self.a, self.b] + list(self.odd.values()):
            self.lib.atmo_destroy(ctx)

    def call(self, entry, o):
        """The entry point with the defaults and the overrides `o` -> (code, [slot name, message] of every slot the call wrote), or None where the
        override is no argument of this entry point."""
        N, lib = self.N, self.lib
        mode_ctx = self.odd[o["mode"]] if "mode" in o else None
        ctx = o["ctx"] if "ctx" in o else (mode_ctx or self.a)
        composite = o.get("composite", 0)

        def one(i, batch):
            """Argument set of the single draw, or of entry i of a batch: the overrides apply to entry 1, o["every"] to all."""
            d = dict(cam=FAR, rect=None, depth=DEPTH, rgba=RGBA + i * STEP, pixels=IMG + i * STEP, fmt=F16, pitch=0, dfmt=D32, texels=TEX + i * STEP, dpitch=0)
            d.update(o.get("every", {}))
            if not batch or i == 1:
                d.update({k: v for k, v in o.items() if k in d})
            f = _frame(d["cam"], d["rect"])
            if "vw" in o and (not batch or i == 1):
                f.viewport_w = o["vw"]
            return f, d, N.AtmoTarget(d["pixels"], d["fmt"], d["pitch"]), N.AtmoDepth(d["texels"], d["dfmt"], d["dpitch"])

        model = None if "model" in o and o["model"] is None else _mat(o.get("model", np.eye(4)))
        size = C.c_float(o.get("size", SIZE))
        if entry in PLANETS:
            arr = (N.AtmoPlanetDraw * 2)()
            for i in range(2):
                f, d, t, _ = one(i, True)
                arr[i].ctx = (o["draw_ctx"] if "draw_ctx" in o else (mode_ctx or self.b)) if i == 1 else self.a
                arr[i].frame, arr[i].depth_dev, arr[i].target = f, d["depth"], t
                arr[i].model_matrix[:] = list(_mat(np.eye(4)) if model is None or i == 0 else model)
                arr[i].box_size = size.value if i == 1 else SIZE
            lst = None if o.get("null_list") else arr
            if "ctx" in o or ("model" in o and o["model"] is None):
                return None   # (the call has no ctx argument and the matrix is no pointer)
            args = (lst, o.get("n", 2), None, None) if entry == "atmo_plan_planets" else (lst, o.get("n", 2), None)
            return self.said(getattr(lib, entry), args, [self.a, arr[1].ctx or self.b], ["draw 0's ctx", "draw 1's ctx"])
        if entry in VIEWS:
            kind = N.AtmoViewDepthTarget if "depth" in entry else N.AtmoViewTarget if "target" in entry else N.AtmoView
            arr = (kind * 2)()
            for i in range(2):
                f, d, t, dep = one(i, True)
                arr[i].frame = f
                if kind is N.AtmoView:
                    arr[i].depth_dev, arr[i].rgba_dev = d["depth"], d["rgba"]
                elif kind is N.AtmoViewTarget:
                    arr[i].depth_dev, arr[i].target = d["depth"], t
                else:
                    arr[i].depth, arr[i].target = dep, t
            lst, n = (None if o.get("null_list") else arr), o.get("n", 2)
            args = (ctx, lst, n, model, size, composite, None) if "proxy" in entry else (ctx, lst, n, composite, None)
            return self.said(getattr(lib, entry), args, [ctx] if ctx else [], ["ctx"])
        f, d, t, dep = one(0, False)
        fp = None if o.get("null_frame") else C.byref(f)
        tp = None if o.get("null_target") else C.byref(t)
        dp = None if o.get("null_depth") else C.byref(dep)
        if entry in ("atmo_render", "atmo_render_composite"):
            args = (ctx, fp, d["depth"], d["rgba"], None)
        elif entry == "atmo_render_tiles":
            args = (ctx, fp, d["depth"], d["rgba"], o.get("tiles", TILES), o.get("n_tiles", 4), None)
        elif entry == "atmo_render_tiles_split":
            args = (ctx, fp, d["depth"], d["rgba"], o.get("tiles", TILES), o.get("n_tiles", 4), o.get("n_heavy", 1), None)
        elif entry == "atmo_render_target":
            args = (ctx, fp, d["depth"], tp, composite, None)
        elif entry == "atmo_render_depth_target":
            args = (ctx, fp, dp, tp, composite, None)
        elif entry in ("atmo_render_proxy", "atmo_render_proxy_composite"):
            args = (ctx, fp, model, size, d["depth"], d["rgba"], None)
        elif entry == "atmo_render_proxy_target":
            args = (ctx, fp, model, size, d["depth"], tp, composite, None)
        else:
            args = (ctx, fp, model, size, dp, tp, composite, None)
        return self.said(getattr(lib, entry), args, [ctx] if ctx else [], ["ctx"])

    def said(self, fn, args, ctxs, names):
        """Another message in every slot first, so that an old one cannot pass; then the call, and what it left where."""
        lib, slots = self.lib, [c for c in ctxs] + [None]
        for ctx in ctxs:
            assert lib.atmo_get_param_f32(ctx, b"no such parameter", None, 0) != self.N.ATMO_OK
        assert lib.atmo_debug_create_host_only(99, 0, 0, 0, 0, C.byref(C.c_void_p())) != self.N.ATMO_OK
        before = [lib.atmo_last_error_string(c) for c in slots]
        rc = fn(*args)
        after = [lib.atmo_last_error_string(c) for c in slots]
        return rc, [(n, (m or b"").decode()) for n, m, m0 in zip(names[:len(ctxs)] + ["no ctx"], after, before) if m != m0]


def _transcript():
    L = _Lib()
    lines, counts = [], {}
    try:
        for entry in ENTRY_POINTS:
            for name, o in _cases(entry):
                got = L.call(entry, o)
                if got is None:
                    continue
                lines.append(" | ".join([entry, name, str(got[0])] + ([f"[{slot}] {msg}" for slot, msg in got[1]] or ["-"])))
                counts[entry] = counts.get(entry, 0) + 1
    finally:
        L.close()
    return lines, counts


def test_every_draw_entry_point_refuses_as_the_golden_transcript_says():
    from godot_atmosphere_shader_amd import _native as N

    lines, counts = _transcript()
    assert set(counts) == set(ENTRY_POINTS) and len(ENTRY_POINTS) == 18 and min(counts.values()) >= 5 and len(lines) >= 120, (counts, len(lines))
    # nothing in the list got as far as a device: a host-only context's draw that does ends as ATMO_E_HIP or ATMO_E_NO_DEVICE
    codes = (str(N.ATMO_OK), str(N.ATMO_E_ARG), str(N.ATMO_E_STATE))
    assert all(line.split(" | ")[2] in codes for line in lines), [line for line in lines if line.split(" | ")[2] not in codes]
    golden = open(GOLDEN).read().splitlines()
    assert golden[0].startswith("# ") and "commit" in golden[0]
    assert lines == golden[1:], "\n".join(f"{a}\n    golden: {b}" for a, b in zip(lines, golden[1:]) if a != b)


if __name__ == "__main__":   # python tests/test_draw_refusals_host.py <commit>, with ATMO_HIP_LIB naming the library built from that commit
    import sys

    assert len(sys.argv) == 2 and os.environ.get("ATMO_HIP_LIB"), "the golden file is written from an older commit's library, never by the code under test"
    text, _ = _transcript()
    with open(GOLDEN, "w") as fh:
        fh.write(f"# {len(text)} calls, written by the library built from commit {sys.argv[1]} (tools/ab_build_commit.sh, ATMO_HIP_LIB): entry point | case | "
                 "code | [slot] message ...\n" + "\n".join(text) + "\n")
