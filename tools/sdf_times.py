"""Times SlotImage.distance_field (csrc/sdf.hip) at 4096^2 on a blob mask: spread 8, spread 64, and spread 64 with wrap,
alternating in one session.  Every round times CALLS calls back to back between two HIP events on the library's stream (profiler
off) and reports us per call, the host's own time per call beside it.  The byte floor of a call is 12 bytes per texel -- 4 read,
the 16-bit intermediate written and read back, 4 written -- at the 6.29 TB/s a float4 copy reaches on this chip; the columns pass
owns 6 of the 12 bytes, the rows pass the other 6.  The split of a call between its two kernels is not visible to events: take it
from a kernel trace of a run of its own (`rocprofv3 --kernel-trace --stats -- python tools/sdf_times.py 2 5`).

    python tools/sdf_times.py [rounds] [calls] [size] [case]          (on the GPU box)        -> profiles/sdf_times.txt
case: 0, 1 or 2 runs that case alone (a kernel trace then holds one spread per kernel name)
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29
CASES = [("spread 8", 8, False), ("spread 64", 64, False), ("spread 64, wrap", 64, True)]


def blob_mask(n, seed=4101):
    """Blobs of many sizes, about 40 % inside: a sum of six products of sinusoids above a threshold (separable, so cheap to make)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f = np.zeros((n, n), np.float32)
    for _ in range(6):
        fy, fx = rng.uniform(2, 24, 2) * 2 * np.pi / n
        f += np.outer(np.sin(t * fy + rng.uniform(0, 6.28)), np.sin(t * fx + rng.uniform(0, 6.28))).astype(np.float32)
    return f > np.float32(0.25)


def main(rounds, calls, n, only=None):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    lib_stream = torch.cuda.ExternalStream(kc.get_stream(), device=torch.device("cuda", 0))

    def timed(fn):
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

    cases = CASES if only is None else [CASES[only]]
    mask = blob_mask(n)
    img = kc.SlotImage.from_planes([mask.astype(np.float32)]).materialize()
    floor_us = 12.0 * n * n / (COPY_TBS * 1e12) * 1e6
    print("distance_field of a %d x %d blob mask (%.1f %% inside), MI355X" % (n, n, 100.0 * mask.mean()))
    print("%d rounds, the cases alternating; each figure: %d calls back to back between two HIP events on the library's stream," % (rounds, calls))
    print("us per call (profiler off); host = the host's own time per call in the same window")
    print("byte floor of a call: 12 B per texel at %.2f TB/s = %.1f us (%.1f us per pass)" % (COPY_TBS, floor_us, floor_us / 2))
    for _, s, wrap in cases:  # warm-up: code objects, the pool's blocks
        for _ in range(3):
            img.distance_field(spread=s, wrap=wrap)
    kc.sync()
    l0, b0 = kc.stats()["kernel_launches"], kc.stats()["algorithmic_bytes"]
    img.distance_field(spread=cases[0][1], wrap=cases[0][2])
    assert kc.stats()["kernel_launches"] - l0 == 2 and kc.stats()["algorithmic_bytes"] - b0 == 12 * n * n
    dev = {name: [] for name, _, _ in cases}
    host = {name: [] for name, _, _ in cases}
    for _ in range(rounds):
        for name, s, wrap in cases:
            d, h = timed(lambda: img.distance_field(spread=s, wrap=wrap))
            dev[name].append(d)
            host[name].append(h)
    for name, _, _ in cases:
        med, lo = statistics.median(dev[name]), min(dev[name])
        print("%-16s median %8.1f us  min %8.1f us  host %6.1f us  = %5.2f x the floor, %5.2f TB/s algorithmic"
              % (name, med, lo, statistics.median(host[name]), med / floor_us, 12.0 * n * n / med / 1e6))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7, int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 4096,
         int(sys.argv[4]) if len(sys.argv) > 4 else None)
