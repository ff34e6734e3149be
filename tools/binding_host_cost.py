"""Host cost per call of the binding's draw methods, this tree against another version of planet_atmosphere.py, with no device: the library is a stub
that answers ATMO_OK and the tensors are the fake CUDA tensors of tests/test_binding_calls_host.py, so what is timed is the Python in front of the C call.

    git show HEAD~1:godot_atmosphere_shader_amd/planet_atmosphere.py > parent_planet_atmosphere.py
    python tools/binding_host_cost.py parent_planet_atmosphere.py

The two versions run in one process, alternating, ROUNDS times; a round's figure is the median of CALLS single calls.  Printed per method: the median
of the rounds' figures and their lowest and highest, for both versions (profiles/binding_refactor/README.md holds one run)."""
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_binding_calls_host as T   # noqa: E402
from godot_atmosphere_shader_amd import planet_atmosphere as new   # noqa: E402

ROUNDS, CALLS = 41, 100


class _Stub:
    def __getattr__(self, name):
        fn = lambda *a: 0   # noqa: E731
        setattr(self, name, fn)
        return fn


def _load(path):
    spec = importlib.util.spec_from_file_location("godot_atmosphere_shader_amd._other_planet_atmosphere", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases(module):
    node = object.__new__(module.PlanetAtmosphere)
    vars(node).update(vars(T._node(lib=_Stub())))
    cam = T._cam()
    depth = T._depth(cam)
    f32, f16 = T._colour("f32", T.H, T.W)[0], T._colour("f16", T.H, T.W)[0]
    cams, depths, _ = T._views(2)
    outs = [c[0] for c in T._view_colours(["f32", "f32"], cams, None, False)]
    return {
        "render": lambda: node.render(cam, depth, f32, stream=T.STREAM),
        "render_composite": lambda: node.render_composite(cam, depth, f32, stream=T.STREAM),
        "render_proxy_composite": lambda: node.render_proxy_composite(cam, depth, f16, stream=T.STREAM),
        "render_views (2 views)": lambda: node.render_views(cams, depths, outs, stream=T.STREAM),
    }


def _round(fn):
    fn()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter_ns()
        fn()
        t.append(time.perf_counter_ns() - t0)
    return statistics.median(t) / 1e3


def main():
    arms = {"other": _cases(_load(sys.argv[1])), "this": _cases(new)}
    figures = {arm: {m: [] for m in cases} for arm, cases in arms.items()}
    for _ in range(ROUNDS):
        for method in arms["this"]:
            for arm in ("other", "this"):
                figures[arm][method].append(_round(arms[arm][method]))
    print("| method | other: median of rounds (lowest .. highest), us | this tree: median (lowest .. highest), us | this - other, us |")
    print("|---|---|---|---|")
    for method in arms["this"]:
        o, n = figures["other"][method], figures["this"][method]
        print(f"| {method} | {statistics.median(o):.1f} ({min(o):.1f} .. {max(o):.1f}) | {statistics.median(n):.1f} ({min(n):.1f} .. {max(n):.1f}) "
              f"| {statistics.median(n) - statistics.median(o):+.1f} |")


if __name__ == "__main__":
    main()
