"""Per-channel statistics at 4096^2 (csrc/stats.hip): kernel time, read bytes and the fraction of 8 TB/s per case -- Gray and
RGBA; min / max only, with the histogram, with the sRGB histogram; random data and one-bin data -- the combine kernel on its own
line, and the wall-clock of kc_image_channel_stats beside kc_image_to_f32 + numpy for the same answer.

    python profiles/channel_stats_times.py run [reps]          (on the GPU box; wall-clock, bytes per call)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/channel_stats_times.py run [reps]
    python profiles/channel_stats_times.py report DIR/.../*_kernel_trace.csv run.log    -> the table (channel_stats_times.txt)

The cases run in a fixed order, each as one warm-up call and `reps` timed calls, so the report assigns the trace's dispatches to
the cases by their order.
"""
import csv
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 4096
PEAK_TBS = 8.0
PX = N * N
# (name, channels, data, histogram, srgb)
CASES = [(("%s %s %s" % ("RGBA" if ch == 4 else "Gray", mode, data)), ch, data, mode != "min/max", mode == "sRGB hist")
         for ch in (1, 4) for data in ("random", "one-bin") for mode in ("min/max", "hist", "sRGB hist")]


def planes_for(ch, data):
    import numpy as np
    rng = np.random.default_rng(ch)
    if data == "random":
        return [rng.random((N, N), dtype=np.float32) for _ in range(ch)]
    return [np.zeros((N, N), np.float32) for _ in range(ch)]  # every pixel in bin 0


def run(reps):
    import numpy as np

    import kanter_core_amd as kc
    kc.init(0)
    imgs = {}
    for ch in (1, 4):
        for data in ("random", "one-bin"):
            imgs[ch, data] = kc.SlotImage.from_planes(planes_for(ch, data)).materialize()
    kc.sync()
    for name, ch, data, hist, srgb in CASES:
        img = imgs[ch, data]
        img.channel_stats(hist, srgb)  # warm-up
        b0 = kc.stats()["algorithmic_bytes"]
        for _ in range(reps):
            img.channel_stats(hist, srgb)
        print("bytes %-28s %d per call" % (name, (kc.stats()["algorithmic_bytes"] - b0) // reps))
    # the same answer (RGBA range, NaN count and histogram) through the host: kc_image_to_f32 + numpy
    img = imgs[4, "random"]
    dev_ms, host_ms = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        img.channel_stats(True)
        dev_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for p in img.planes():
            ok = p[~np.isnan(p)]
            ok.min(), ok.max()
            np.bincount((np.clip(p, 0, 1) * np.float32(255)).astype(np.uint8).reshape(-1), minlength=256)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    print("wall RGBA kc_image_channel_stats (histogram):  median %.3f ms" % statistics.median(dev_ms))
    print("wall RGBA kc_image_to_f32 + numpy (same answer): median %.3f ms" % statistics.median(host_ms))
    print("reps %d" % reps)


def report(trace_csv, log):
    lines = open(log).read().splitlines()
    reps = int(next(x.split()[1] for x in lines if x.startswith("reps ")))
    rows = list(csv.DictReader(open(trace_csv)))
    col = lambda key: next(k for k in rows[0] if key in k)  # noqa: E731
    kn, ks, ke = col("Kernel_Name"), col("Start_Timestamp"), col("End_Timestamp")
    rows.sort(key=lambda r: int(r[ks]))
    mains = [int(r[ke]) - int(r[ks]) for r in rows if "channel_stats_kernel" in r[kn]]
    combs = [int(r[ke]) - int(r[ks]) for r in rows if "channel_stats_combine_kernel" in r[kn]]
    per = reps + 1
    # the cases' dispatches come first; the wall-clock comparison's calls follow them
    assert len(mains) >= len(CASES) * per and len(combs) == len(mains), (len(mains), len(combs))
    out = ["Channel statistics, %d x %d, MI355X; kernel times from rocprofv3 --kernel-trace (median of %d calls after a warm-up), "
           "fraction of %.0f TB/s = read bytes / time / peak" % (N, N, reps, PEAK_TBS), ""]
    out.append("%-30s %10s %9s %9s %12s" % ("case", "median us", "MB read", "of 8TB/s", "combine us"))
    for i, (name, ch, _, _, _) in enumerate(CASES):
        ns = statistics.median(mains[i * per + 1:(i + 1) * per])
        cns = statistics.median(combs[i * per + 1:(i + 1) * per])
        b = 4 * ch * PX
        out.append("%-30s %10.1f %9.1f %9.3f %12.1f" % (name, ns / 1e3, b / 1e6, b / ns / 1e3 / PEAK_TBS, cns / 1e3))
    out.append("")
    out.append("Algorithmic bytes per call (kc_stats_algorithmic_bytes) and wall-clock (a run of its own, without the tracer):")
    out += ["  " + x.rstrip() for x in lines if x.startswith(("bytes ", "wall "))]
    print("\n".join(out))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        report(sys.argv[2], sys.argv[3])
