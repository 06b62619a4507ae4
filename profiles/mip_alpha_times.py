"""Alpha-weighted mip chains at 4096^2 (csrc/mip_alpha.hip, KC_MIP_ALPHA_WEIGHT) beside the plain chain of the same image,
alternating in one session, on an RGBA image of four resident planes under two alphas --
    dots    a dot mask of about 30 %: seven texels in ten are unknown at level 0 and walk up to an ancestor in the push,
    opaque  a resident alpha of ones: every texel is known, the push reads the weights and writes nothing
-- in the forms
    (a) mips(): the yardstick, the plain chain of the four planes,
    (b) mips(alpha_weighted=True): the pull (two launches), the push (one) and alpha's plain chain (two).
Every round times CALLS calls back to back between two HIP events on the library's stream (profiler off) and reports us per
call; the host's own time per call is printed beside it.  The rate is kc_stats' algorithmic bytes over the median; for (b) they
do not hold what the push writes (12 bytes per unknown texel, and the ancestors' weights it walks), which is printed beside it
from the data.  Also: (b) == its KC_MIP_PER_LEVEL form byte for byte at full size.

    python profiles/mip_alpha_times.py [rounds] [calls]          (on the GPU box)        -> profiles/mip_alpha_times.txt
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

    rng = np.random.default_rng(4099)
    colour = [rng.random((N, N), dtype=np.float32) for _ in range(3)]
    y, x = np.mgrid[0:N, 0:N]
    dx, dy = (x + 2) % 10 - 4.5, (y + 2) % 10 - 4.5
    dots = (dx * dx + dy * dy < 9.0).astype(np.float32)
    del x, y, dx, dy
    colour[0] = np.where(dots > 0, np.float32(0.8), np.float32(0.0)).astype(np.float32)  # R: the cutout's colour on black
    images = [("dots", kc.SlotImage.from_planes(colour + [dots]).materialize(), 1.0 - float(dots.mean())),
              ("opaque", kc.SlotImage.from_planes(colour + [np.ones((N, N), np.float32)]).materialize(), 0.0)]
    print("Alpha-weighted mip chains of a %d x %d image of four resident planes, MI355X" % (N, N))
    print("%d rounds, the forms alternating; each figure: %d calls back to back between two HIP events on the library's stream,"
          % (rounds, calls))
    print("us per call (profiler off); host = the host's own time per call in the same window")
    print()
    for name, img, unknown in images:
        forms = [("(a) plain", lambda: img.mips()), ("(b) alpha-weighted", lambda: img.mips(alpha_weighted=True))]
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
        print("  alpha: %s (%.1f %% of level 0 unknown)" % (name, 100.0 * unknown))
        for f, _ in forms:
            r = runs[f]
            print("    %-20s %s   range %.1f - %.1f   median %.1f   host median %.1f   (%d launches, %.1f MB algorithmic)" % (
                f, " ".join("%7.1f" % v for v in r), min(r), max(r), statistics.median(r), statistics.median(hosts[f]), algs[f][0],
                algs[f][1] / 1e6))
        a, b = (runs[f] for f, _ in forms)
        rate = [algs[f][1] / (statistics.median(runs[f]) * 1e-6) / 1e12 / PEAK_TBS for f, _ in forms]
        print("    by algorithmic bytes: (a) %.3f of %.0f TB/s, (b) %.3f: %.2f of (a)'s rate;  (b) per level-0 texel: %.1f B, and %.1f B"
              " more that the push writes at level 0" % (rate[0], PEAK_TBS, rate[1], rate[1] / rate[0], algs[forms[1][0]][1] / (N * N), 12.0 * unknown))
        fused, per_level = img.mips(alpha_weighted=True), img.mips(alpha_weighted=True, per_level=True)
        for k, (p, q) in enumerate(zip(fused, per_level)):
            for u, v in zip(p.planes(), q.planes()):
                assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), k
        print("    (b) == its per-level form byte for byte, %d levels; mean R of levels 0, 2, 6: %s (plain: %s)" % (
            len(fused), ", ".join("%.3f" % float(fused[k].planes()[0].mean()) for k in (0, 2, 6)),
            ", ".join("%.3f" % float(lv.planes()[0].mean()) for lv in [img.mips()[k] for k in (0, 2, 6)])))
        print()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
