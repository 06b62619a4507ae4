"""Alpha-test coverage at 4096^2 (csrc/mip_coverage.hip): mips() against mips(coverage=128) of the same RGBA image of four resident
planes, once with a noise alpha (no ties: every 10-bit bin is hit) and once with a 0/1 dot mask (every wave's texels fall in one
or two bins: the case hist_add's wave-uniform shortcut is there for).  mips() without the flag runs the code it ran before the
flag existed, so it stands for the chain as it was.  The forms alternate; every round times CALLS calls back to back between two
HIP events on the library's stream (profiler off) and reports us per call, with the host's own time per call beside it.

    python profiles/mip_coverage_times.py [rounds] [calls]          (on the GPU box)        -> profiles/mip_coverage_times.txt
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4096
REF = 128


def main(rounds, calls):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    lib_stream = torch.cuda.ExternalStream(kc.get_stream(), device=torch.device("cuda", 0))

    def timed(fn, img):
        kc.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(lib_stream)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(img)
        host = time.perf_counter() - t0
        e1.record(lib_stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls, host * 1e6 / calls

    print("Mip chains of a %d x %d RGBA image of four resident planes with KC_MIP_COVERAGE_REF(%d), MI355X" % (N, N, REF))
    print("%d rounds, the forms alternating; each figure: %d calls back to back between two HIP events on the library's stream,"
          % (rounds, calls))
    print("us per call (profiler off); host = the host's own time per call in the same window")
    print()
    rng = np.random.default_rng(4098)
    rgb = [rng.random((N, N), dtype=np.float32) for _ in range(3)]
    alphas = {"noise alpha": rng.random((N, N), dtype=np.float32), "0/1 dot mask (30 %)": (rng.random((N, N)) < 0.3).astype(np.float32)}
    forms = [("plain", lambda i: i.mips()), ("coverage", lambda i: i.mips(coverage=REF)),
             ("coverage, per level", lambda i: i.mips(per_level=True, coverage=REF))]
    medians = {}
    for name, alpha in alphas.items():
        img = kc.SlotImage.from_planes(rgb + [alpha]).materialize()
        for _, fn in forms:  # warm-up: code objects, pool blocks
            fn(img)
            fn(img)
        kc.sync()
        runs = {f: [] for f, _ in forms}
        hosts = {f: [] for f, _ in forms}
        for _ in range(rounds):
            for f, fn in forms:
                dev, host = timed(fn, img)
                runs[f].append(dev)
                hosts[f].append(host)
        l0 = kc.stats()
        img.mips()
        l1 = kc.stats()
        img.mips(coverage=REF)
        l2 = kc.stats()
        extra_launches = (l2["kernel_launches"] - l1["kernel_launches"]) - (l1["kernel_launches"] - l0["kernel_launches"])
        extra_bytes = (l2["algorithmic_bytes"] - l1["algorithmic_bytes"]) - (l1["algorithmic_bytes"] - l0["algorithmic_bytes"])
        info = img.mip_coverage_info(REF)
        print("%s (plain: %d launches; the flag adds %d launches and %.1f MB algorithmic; %d of %d levels scaled)" % (
            name, l1["kernel_launches"] - l0["kernel_launches"], extra_launches, extra_bytes / 1e6,
            sum(i.scale != 1.0 for i in info), len(info) - 1))
        for f, _ in forms:
            r = runs[f]
            medians[name, f] = statistics.median(r)
            print("  %-20s %s   range %.1f - %.1f   median %.1f   host median %.1f" % (
                f, " ".join("%7.1f" % x for x in r), min(r), max(r), statistics.median(r), statistics.median(hosts[f])))
        extra = medians[name, "coverage"] - medians[name, "plain"]
        print("  coverage - plain, medians: %.1f us;  the flag's bytes over that time: %.2f TB/s" % (extra, extra_bytes / (extra * 1e-6) / 1e12))
        # the levels against the share of level 0, as a renderer's test sees them
        plain, kept = img.mips(), img.mips(coverage=REF)
        share = lambda lv: lv.alpha_coverage(REF) / (lv.size().width * lv.size().height)  # noqa: E731
        print("  covered share, levels 0-5: plain %s;  with the flag %s" % (
            " ".join("%.3f" % share(lv) for lv in plain[:6]), " ".join("%.3f" % share(lv) for lv in kept[:6])))
        print()
    names = list(alphas)
    a = medians[names[0], "coverage"] - medians[names[0], "plain"]
    b = medians[names[1], "coverage"] - medians[names[1], "plain"]
    print("the flag's cost, mask over noise: %.2f" % (b / a))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
