"""Roughness mip chains at 4096^2 (csrc/mip_roughness.hip, kc_image_build_roughness_mips) in three forms, alternating in one
session --
    (a) the fused roughness chain of a Gray roughness plane beside a kc_height_to_normal_process result (two launches),
    (b) the same with KC_MIP_PER_LEVEL (twelve launches of the one-level kernel),
    (c) the yardstick: the plain chain of an RGBA image of four resident planes, which reads the same four planes and writes
        four times as much
-- every round times CALLS calls back to back between two HIP events on the library's stream (profiler off) and reports us per
call; the host's own time per call is printed beside it.  Also: (a) == (b) byte for byte at full size, and how far the chain
lies above the plain chain of the same roughness plane.

    python profiles/mip_roughness_times.py [rounds] [calls]          (on the GPU box)        -> profiles/mip_roughness_times.txt
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4096
PEAK_TBS = 8.0


def main(rounds, calls):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    lib_stream = torch.cuda.ExternalStream(kc.get_stream(), device=torch.device("cuda", 0))

    def timed(fn):
        """us per call on the device's clock and on the host's"""
        kc.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(lib_stream)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        host = time.perf_counter() - t0
        e1.record(lib_stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls, host * 1e6 / calls

    rng = np.random.default_rng(4098)
    plane = lambda: rng.random((N, N), dtype=np.float32)  # noqa: E731
    normals = kc.height_to_normal_process(kc.SlotImage.from_planes([plane()]))
    rho = kc.SlotImage.from_planes([plane()]).materialize()
    rgba = kc.SlotImage.from_planes([plane() for _ in range(4)]).materialize()
    forms = [("(a) roughness, fused", lambda: rho.roughness_mips(normals)),
             ("(b) roughness, per level", lambda: rho.roughness_mips(normals, per_level=True)),
             ("(c) plain, four planes", lambda: rgba.mips())]
    print("Roughness mip chains of a %d x %d image, MI355X" % (N, N))
    print("%d rounds, the forms alternating; each figure: %d calls back to back between two HIP events on the library's stream,"
          % (rounds, calls))
    print("us per call (profiler off); host = the host's own time per call in the same window")
    print()
    for _, fn in forms:  # warm-up: code objects, pool blocks
        fn()
        fn()
    kc.sync()
    runs = {f: [] for f, _ in forms}
    hosts = {f: [] for f, _ in forms}
    for _ in range(rounds):
        for f, fn in forms:
            dev, host = timed(fn)
            runs[f].append(dev)
            hosts[f].append(host)
    algs = {}
    for f, fn in forms:
        l0 = kc.stats()
        fn()
        l1 = kc.stats()
        algs[f] = (l1["kernel_launches"] - l0["kernel_launches"], l1["algorithmic_bytes"] - l0["algorithmic_bytes"])
    for f, _ in forms:
        r = runs[f]
        print("  %-26s %s   range %.1f - %.1f   median %.1f   host median %.1f   (%d launches, %.1f MB algorithmic)" % (
            f, " ".join("%7.1f" % x for x in r), min(r), max(r), statistics.median(r), statistics.median(hosts[f]), algs[f][0], algs[f][1] / 1e6))
    a, b, c = (runs[f] for f, _ in forms)
    spread = max(c) - min(c)
    print("  (a) wholly below (b): %s;  (a) above (c)'s range by %.1f us, (c)'s own spread %.1f us: %s" % (
        "yes" if max(a) < min(b) else "NO", max(0.0, max(a) - max(c)), spread, "within" if max(a) - max(c) <= spread else "ABOVE"))
    print("  (a) by algorithmic bytes: %.3f of %.0f TB/s;  (c): %.3f" % (
        algs[forms[0][0]][1] / (statistics.median(a) * 1e-6) / 1e12 / PEAK_TBS, PEAK_TBS,
        algs[forms[2][0]][1] / (statistics.median(c) * 1e-6) / 1e12 / PEAK_TBS))
    fused, per_level, plain = rho.roughness_mips(normals), rho.roughness_mips(normals, per_level=True), rho.mips()
    means = []
    for k, (x, y, z) in enumerate(zip(fused, per_level, plain)):
        p, q = x.planes()[0], y.planes()[0]
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), k
        means.append((float(p.mean()), float(z.planes()[0].mean())))
    print("  (a) == (b) byte for byte, %d levels; mean roughness of levels 1, 3, 6: %s (plain: %s)" % (
        len(fused), ", ".join("%.3f" % means[k][0] for k in (1, 3, 6)), ", ".join("%.3f" % means[k][1] for k in (1, 3, 6))))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
