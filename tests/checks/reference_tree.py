#!/usr/bin/env python3
"""The committed vectors against the reference's own shader text, re-executed: what tests/ pins to tests/golden/*.npz is checked here against
its source, the reference checkout (addons/zylann.atmosphere/shaders), which this repository does not contain -- so it is a check to run by
hand where a reference checkout and Mesa are present, not part of the suite.

  1. a sample of reference_exec.npz (one bake, one clouds_high_rm frame) re-executed from the text by tests/golden/gdshader_vm.py: the same bits;
  2. what tests/golden/mesa_exec.py hands to Mesa's compiler is the reference's text, every changed line one of four declared edits;
  3. the same sample of reference_exec_mesa.npz compiled by Mesa again and drawn by llvmpipe: the same bits (needs Mesa's swrast driver).

    python tests/checks/reference_tree.py <reference checkout>"""
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

from godot_atmosphere_shader_amd import scene as S  # noqa: E402
import reference_scenes as RS  # noqa: E402


def textures():
    return dict(blue_noise=S.make_blue_noise(), shape=S.make_shape_texture(RS.SHAPE_N), cubemap=S.make_coverage_cubemap(RS.CUBE_N))


def vectors_reproduce_from_the_reference_tree(shaders):
    """Re-execute a sample of the vectors from the reference's source."""
    import make_reference_vectors as G
    import vm_textures as T
    from oracle.oracle import Oracle

    G.SHADERS = shaders
    vectors = np.load(os.path.join(GOLDEN, "reference_exec.npz"))
    oracle32 = Oracle("f32")
    lut, _ = G.run_bake(RS.scenes()["alt"][0])
    assert np.array_equal(lut.view(np.uint32), vectors["lut_alt"].view(np.uint32))
    params, model = RS.scenes()["alt"]
    tex = textures()
    cube = tex["cubemap"]
    padded = T.pad_cubemap(cube, lambda f, i, j: oracle32.cube_texel(cube, f, i, j))
    units = dict(u_optical_depth_texture=T.LutTexture(lut), u_blue_noise_texture=T.ByteTexture2D(tex["blue_noise"]),
                 u_cloud_shape_texture=T.ShapeTexture(tex["shape"]), u_cloud_coverage_cubemap=T.CubeTexture(padded))
    cam = RS.camera_from_fixture(vectors, RS.W, RS.H, "P_clouds")
    rgba, _, _, _ = G.run_frame("planet_atmosphere_clouds_high_rm", None, params, np.linalg.inv(model), model, cam,
                                vectors["depth_alt_P_clouds"], units)
    assert np.array_equal(rgba, vectors["rgba_alt_P_clouds_planet_atmosphere_clouds_high_rm"])


def what_mesa_compiles_is_the_references_text(shaders):
    """mesa_exec.translate: between the prelude it puts in front (the #version line, the engine built-ins) and the main() it appends, the source handed to
    Mesa's compiler is the reference's files with their #includes pasted in, and every line that differs from the file on disk is one of the four
    declared edits: a `uniform` declaration stripped of hints and default, a `varying` turned into a global, a `shader_type` / `render_mode` line
    dropped, a trailing comma removed in front of `)`.  No statement inside a function body is touched."""
    import mesa_exec as M

    M.SHADERS = shaders
    names = sorted(f for f in os.listdir(M.SHADERS) if f.endswith(".gdshader"))
    assert len(names) == 8
    edited = {"uniform": 0, "varying": 0, "dropped": 0, "comma": 0}
    total = 0
    for f in names:
        path = os.path.join(M.SHADERS, f)
        original = M.flatten(path, {}).split("\n")
        for stage in ("fragment", "vertex") if "planet_atmosphere" in f else ("canvas",):
            src, _ = M.translate(path, stage=stage)
            begin = src.index("out vec4 MGL_out;\n") + len("out vec4 MGL_out;\n")
            body = src[begin:src.rindex("\nvoid main() {")].split("\n")
            assert len(body) == len(original), f
            for k, (a, b) in enumerate(zip(original, body)):
                total += 1
                if a == b:
                    continue
                if re.match(r"\s*uniform\s", a):
                    ty, name = re.match(r"\s*uniform\s+(\w+)\s+(\w+)", a).groups()
                    assert b.strip() == f"uniform {ty} {name};", (a, b)     # hints and default gone, nothing else
                    edited["uniform"] += 1
                elif re.match(r"\s*varying\s", a):
                    assert b.strip() == a.strip()[len("varying"):].strip(), (a, b)
                    edited["varying"] += 1
                elif re.match(r"\s*(shader_type|render_mode)\b", a):
                    assert re.sub(r"^\s*(shader_type|render_mode)\b[^;]*;", "", a) == b, (a, b)
                    edited["dropped"] += 1
                else:
                    # a trailing comma in front of `)`: on this line, or at its end with the `)` opening the next line
                    same_line = re.sub(r",(\s*)\)", r"\1)", a)
                    line_end = (a.rstrip()[:-1] + a[len(a.rstrip()):]) if a.rstrip().endswith(",") and original[k + 1].lstrip().startswith(")") else None
                    assert b in (same_line, line_end), (a, b)
                    edited["comma"] += 1
    print(f"{total} lines of reference text handed to Mesa over {len(names)} shaders x stages; edited: {edited}")
    assert edited["uniform"] > 100 and edited["varying"] > 10 and edited["dropped"] > 10 and 0 < edited["comma"] < 400


def mesa_vectors_reproduce_here(shaders):
    """Compile the text again, draw one frame and one bake: the same bits as the committed Mesa vectors."""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import mesa_exec as M, reference_scenes as RS; M.SHADERS = %r;"
            "from godot_atmosphere_shader_amd import scene as S; z = np.load(%r); m = np.load(%r); p, model = RS.scenes()['alt'];"
            "tex = dict(lut=z['lut_alt'], blue=S.make_blue_noise(), shape=S.make_shape_texture(RS.SHAPE_N), cubemap=S.make_coverage_cubemap(RS.CUBE_N));"
            "cam = RS.camera_from_fixture(z, RS.W, RS.H, 'P_clouds');"
            "rgba, disc, vary = M.run_frame('planet_atmosphere_clouds_high_rm', None, p, np.linalg.inv(model), model, cam, z['depth_alt_P_clouds'], tex);"
            "assert np.array_equal(rgba, m['rgba_alt_P_clouds_planet_atmosphere_clouds_high_rm']);"
            "lut, _ = M.run_bake(p); assert np.array_equal(lut.view(np.uint32), m['lut_alt'].view(np.uint32)); print('same bits')"
            % (ROOT, GOLDEN, shaders, os.path.join(GOLDEN, "reference_exec.npz"), os.path.join(GOLDEN, "reference_exec_mesa.npz")))
    # (a process of its own: llvmpipe's worker threads and LLVM's JIT stay out of this one)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "same bits" in r.stdout, r.stderr[-2000:]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__.rsplit("\n", 1)[-1].strip())
    shaders = os.path.join(os.path.abspath(sys.argv[1]), "addons", "zylann.atmosphere", "shaders")
    if not os.path.isdir(shaders):
        raise SystemExit(f"{shaders}: not a reference checkout")
    for check in (vectors_reproduce_from_the_reference_tree, what_mesa_compiles_is_the_references_text, mesa_vectors_reproduce_here):
        check(shaders)
        print(f"{check.__name__}: ok")


if __name__ == "__main__":
    main()
