"""Times SlotImage.blur (csrc/blur.hip) at 4096^2, Gray and RGBA, for R = 3, 12 and 64 (sigma 1.0, 4.0, 21.3), clamped and with
wrap: the rows pass alone (sigma_y = 0), the columns pass alone (sigma_x = 0) and both, beside a one-step Mix(Add) of the same
planes in the same session -- the stream rate to judge them by: a Mix moves 12 bytes per texel and plane, a blur pass 8.  Every
figure is CALLS calls back to back between two HIP events on the library's stream (profiler off), the median of ROUNDS rounds
with the cases alternating.  "warm": one source again and again under the default cache policy (a Gray source, 64 MiB, stays in
the Infinity Cache).  "cold": the calls rotate over sources of 768 MiB in all, so that no call finds its source in the cache.

    python tools/blur_times.py [rounds] [calls] [size]          (on the GPU box)        -> profiles/blur_times.txt
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMAS = [(3, 1.0), (12, 4.0), (64, 21.3)]


def main(rounds, calls, n):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    lib_stream = torch.cuda.ExternalStream(kc.get_stream(), device=torch.device("cuda", 0))

    def timed(fn):
        kc.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(lib_stream)
        for i in range(calls):
            fn(i)
        e1.record(lib_stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    rng = np.random.default_rng(4201)
    print("blur of %d x %d images, MI355X; %d rounds, the cases alternating; each figure: the median over the rounds of %d calls back"
          % (n, n, rounds, calls))
    print("to back between two HIP events on the library's stream, us per call (profiler off).  rate: 8 B per texel and plane per pass")
    print("(12 for the Mix); 'of mix': that rate over the rate of the one-step Mix(Add) of the same planes, timed in the same rounds")
    for kind, planes in (("gray", 1), ("rgba", 4)):
        count = {"warm": 1, "cold": max(2, -(-768 * 2 ** 20 // (planes * n * n * 4)))}
        for temp in ("warm", "cold"):
            srcs = [kc.SlotImage.from_planes([rng.random((n, n), dtype=np.float32) for _ in range(planes)]).materialize()
                    for _ in range(count[temp] + 1)]
            m = len(srcs) - 1  # the last one is only the Mix's other side
            cases = [("mix", lambda i: kc.mix_process(srcs[i % m], srcs[m], kc.MixType.Add).materialize(), 12.0)]
            for R, s in SIGMAS:
                for wrap in (False, True):
                    tag = "R %2d %s" % (R, "wrap " if wrap else "clamp")
                    cases.append((tag + " rows", lambda i, s=s, wrap=wrap: srcs[i % m].blur(s, 0.0, wrap=wrap), 8.0))
                    cases.append((tag + " columns", lambda i, s=s, wrap=wrap: srcs[i % m].blur(0.0, s, wrap=wrap), 8.0))
                    cases.append((tag + " both", lambda i, s=s, wrap=wrap: srcs[i % m].blur(s, wrap=wrap), 16.0))
            for _, fn, _ in cases:  # warm-up: code objects, the pool's blocks
                fn(0)
                fn(1)
            kc.sync()
            us = {name: [] for name, _, _ in cases}
            for _ in range(rounds):
                for name, fn, _ in cases:
                    us[name].append(timed(fn))
            mix_rate = 12.0 * planes * n * n / statistics.median(us["mix"]) / 1e6
            print("%s, %s (%d source%s):" % (kind, temp, m, "" if m == 1 else "s"))
            for name, _, b in cases:
                med = statistics.median(us[name])
                rate = b * planes * n * n / med / 1e6
                print("  %-22s median %9.1f us  min %9.1f us  %5.2f TB/s  %5.2f of mix" % (name, med, min(us[name]), rate, rate / mix_rate))
            del srcs, cases
            kc.sync()
            kc.pool_trim()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 10, int(sys.argv[3]) if len(sys.argv) > 3 else 4096)
