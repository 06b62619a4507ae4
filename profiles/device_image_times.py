"""Device-memory image conversions at 4096^2 RGBA (csrc/devimage.hip): kernel time, algorithmic bytes and the fraction of 8 TB/s
per case, beside the u8 kernels of the host path (to_u8_kernel / from_u8_kernel) and the wall-clock of the host and device paths
for the same U8 import / export pair.

    python profiles/device_image_times.py run [reps]          (on the GPU box; wall-clock of the two paths, bytes per call)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/device_image_times.py run [reps]
    python profiles/device_image_times.py report DIR/.../*_kernel_stats.csv run.log    -> the table (device_image_times.txt)
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
# case -> (kernel name fragment in the trace, algorithmic bytes per pixel)
CASES = [
    ("U8 HWC RGBA import", "image_import_kernel<0, 0,", 4 + 16),
    ("U8 HWC RGBA export", "image_export_kernel<0, 0, false,", 16 + 4),
    ("U8 HWC RGBA export sRGB", "image_export_kernel<0, 0, true,", 16 + 4),
    ("F16 HWC RGBA import", "image_import_kernel<2, 0,", 8 + 16),
    ("F16 HWC RGBA export", "image_export_kernel<2, 0, false,", 16 + 8),
    ("F32 CHW RGBA import", "image_import_kernel<4, 1,", 16 + 16),
    ("F32 CHW RGBA export", "image_export_kernel<4, 1, false,", 16 + 16),
    ("host path: from_u8_kernel (RGBA)", "from_u8_kernel", 4 + 16),
    ("host path: to_u8_kernel", "to_u8_kernel<false,", 16 + 4),
    ("host path: to_u8_kernel sRGB", "to_u8_kernel<true,", 16 + 4),
]


def run(reps):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    rng = np.random.default_rng(1)
    px = rng.integers(0, 256, size=(N, N, 4), dtype=np.uint8)
    t8 = torch.from_numpy(px).cuda()
    img = kc.SlotImage.from_u8(px).materialize()
    t16 = torch.empty((N, N, 4), dtype=torch.float16, device="cuda").copy_(t8)
    t32 = torch.empty((4, N, N), dtype=torch.float32, device="cuda").copy_(t8.permute(2, 0, 1))
    o8 = torch.empty((N, N, 4), dtype=torch.uint8, device="cuda")
    o16 = torch.empty((N, N, 4), dtype=torch.float16, device="cuda")
    o32 = torch.empty((4, N, N), dtype=torch.float32, device="cuda")
    steps = [
        ("U8 HWC RGBA import", lambda: kc.SlotImage.from_torch(t8)),
        ("U8 HWC RGBA export", lambda: img.to_torch(out=o8)),
        ("U8 HWC RGBA export sRGB", lambda: img.to_torch(out=o8, srgb=True)),
        ("F16 HWC RGBA import", lambda: kc.SlotImage.from_torch(t16)),
        ("F16 HWC RGBA export", lambda: img.to_torch(out=o16)),
        ("F32 CHW RGBA import", lambda: kc.SlotImage.from_torch(t32, layout="chw")),
        ("F32 CHW RGBA export", lambda: img.to_torch(layout="chw", out=o32)),
        ("host path: to_u8 (kernel + copy to host)", lambda: img.to_u8()),
        ("host path: to_u8_srgb", lambda: img.to_u8(True)),
    ]
    for name, fn in steps:
        fn()  # warm-up
        torch.cuda.synchronize()
        kc.sync()
        b0 = kc.stats()["algorithmic_bytes"]
        keep = [fn() for _ in range(reps)]
        kc.sync()
        torch.cuda.synchronize()
        print("bytes %-42s %d per call" % (name, (kc.stats()["algorithmic_bytes"] - b0) // reps))
        del keep
    # the same U8 RGBA import / export pair by the two paths, wall-clock, synchronised at the end of each pair
    host_ms, dev_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        a = kc.SlotImage.from_u8(px)
        a.to_u8()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = kc.SlotImage.from_torch(t8)
        d.to_torch(out=o8)
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    print("pair host path (kc_image_from_u8 + kc_image_to_u8, host buffers): median %.3f ms" % statistics.median(host_ms))
    print("pair device path (from_torch + to_torch, device buffers):          median %.3f ms" % statistics.median(dev_ms))


def report(stats_csv, log):
    rows = list(csv.DictReader(open(stats_csv)))
    out = ["Device-memory image conversions, %d x %d RGBA, MI355X; kernel times from rocprofv3 --kernel-trace --stats (average "
           "over the calls), fraction of %.0f TB/s = algorithmic bytes / time / peak" % (N, N, PEAK_TBS), ""]
    out.append("%-36s %8s %10s %9s %8s" % ("case", "calls", "avg us", "MB", "of 8TB/s"))
    for name, frag, bpp in CASES:
        hit = [r for r in rows if frag in r["Name"]]
        if not hit:
            out.append("%-36s not measured (kernel not in the trace)" % name)
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        ns = sum(float(r["TotalDurationNs"]) for r in hit) / calls
        mb = bpp * PX / 1e6
        out.append("%-36s %8d %10.1f %9.1f %8.3f" % (name, calls, ns / 1e3, mb, bpp * PX / ns / 1e3 / PEAK_TBS))
    out.append("")
    out.append("Algorithmic bytes per call (kc_stats_algorithmic_bytes) and wall-clock of the U8 import / export pair (a run of its own,")
    out.append("without the tracer):")
    out += ["  " + line.rstrip() for line in open(log) if line.startswith(("bytes ", "pair "))]
    print("\n".join(out))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        report(sys.argv[2], sys.argv[3])
