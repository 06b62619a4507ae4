"""Block compression at 4096^2 (csrc/bc.hip, csrc/bc7.hip, csrc/bc6h.hip): kernel time, algorithmic bytes and the fraction of 8 TB/s
per case -- Gray BC4; RGBA BC1, BC1 sRGB, BC3, BC3 sRGB, BC4, BC5, BC7 and BC7 sRGB; BC6H encode, decode and compare (of its own
blocks) on planes over [0, 8); random data and a uniform image (every block takes the
d == 0 / c0 == c1 path; BC7 and BC6H search their palettes all the same)
-- and BC1 with punch-through alpha (csrc/bc1a.hip, KC_BC_PUNCH_THROUGH at byte 128), linear and sRGB, on random alpha (nearly
every block mixed: the worst case) and on a cutout of a few large disks (mostly full and empty blocks: the shipping case)
-- with kc_image_to_device U8 of the same images beside them as the yardstick, and the wall-clock of kc_image_to_bc against
kc_image_to_u8 plus the numpy reference encoder (tests/bc_ref.py) for the same blocks.

    python profiles/bc_times.py run [reps]          (on the GPU box; wall-clock, bytes per call)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/bc_times.py run [reps]
    python profiles/bc_times.py report DIR/.../*_kernel_trace.csv run.log    -> the table (bc_times.txt)

The cases run in a fixed order, each as one warm-up call and `reps` timed calls, so the report assigns the trace's dispatches to
the cases by their order.

The all-modes decoders (KC_BC_ALL_MODES, csrc/bc_modes.hip) against the single-subset ones, in the same way and in one session,
the two forms alternating: decode and compare of BC7 and BC6H, on the library's own blocks (both forms give the same image) and
on tests/bc_modes_ref.py's random blocks of every (mode, partition) pair (the default form leaves the partitioned ones black).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/bc_times.py modes-run [reps]
    python profiles/bc_times.py modes-report DIR/.../*_kernel_trace.csv run.log    -> the table at the end of bc_decode_times.txt
"""
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4096
PEAK_TBS = 8.0
PX = N * N
BC7 = 98  # KC_BC7
BC6H = 95  # KC_BC6H
BLOCK_BYTES = {1: 8, 3: 16, 4: 8, 5: 16, BC6H: 16, BC7: 16}
PLANES = {1: 3, 3: 4, 4: 1, 5: 2, BC6H: 3, BC7: 4}  # RGBA planes each format reads
# (name, channels, data, kind, fmt, srgb); kind "bc", "u8" (kc_image_to_device U8, the yardstick), or BC6H's "decode" (the
# image's own blocks back to three planes) and "compare" (the image against its own blocks: two launches, the first is timed)
CASES = []
for _data in ("random", "uniform"):
    CASES.append(("Gray BC4 %s" % _data, 1, _data, "bc", 4, False))
    for _fmt, _srgb in ((1, False), (1, True), (3, False), (3, True), (4, False), (5, False), (BC7, False), (BC7, True)):
        CASES.append(("RGBA BC%d%s %s" % (7 if _fmt == BC7 else _fmt, " sRGB" if _srgb else "", _data), 4, _data, "bc", _fmt, _srgb))
    CASES.append(("RGBA to_device U8 %s" % _data, 4, _data, "u8", 0, False))
    for _kind in ("bc", "decode", "compare"):
        CASES.append(("HDR BC6H %s %s" % ("encode" if _kind == "bc" else _kind, _data), 4, "hdr " + _data, _kind, BC6H, False))
PT_REF = 128  # the reference byte of the punch-through cases
for _data in ("cutout random", "cutout disks"):  # kind "pt": BC1 under KC_BC_PUNCH_THROUGH_REF(PT_REF), which reads alpha too
    for _srgb in (False, True):
        CASES.append(("RGBA BC1a%s %s" % (" sRGB" if _srgb else "", _data.split()[1]), 4, _data, "pt", 1, _srgb))
CUTOUTS = ("cutout random", "cutout disks")
OWN = ("hdr random", "hdr uniform")  # the images whose own BC6H blocks decode and compare read: encoded once, before the cases
KERNEL = {"u8": "image_export_kernel", "decode": "bc6h_decode_kernel", "compare": "bc6h_compare_kernel", "pt": "bc1a_encode_kernel"}


def planes_for(ch, data):
    import numpy as np
    rng = np.random.default_rng(ch)
    if data == "cutout disks":  # random colour under five large soft-edged disks of alpha: most blocks lie wholly inside or outside
        y, x = np.mgrid[0:N, 0:N].astype(np.float32)
        alpha = np.zeros((N, N), np.float32)
        for cx, cy, r in ((0.25, 0.3, 0.2), (0.7, 0.25, 0.18), (0.5, 0.6, 0.22), (0.2, 0.8, 0.15), (0.8, 0.8, 0.17)):
            alpha = np.maximum(alpha, np.clip((r * N - np.hypot(x - cx * N, y - cy * N)) / 8.0 + 0.5, 0.0, 1.0))
        return [rng.random((N, N), dtype=np.float32) for _ in range(3)] + [alpha.astype(np.float32)]
    scale = np.float32(8.0 if data.startswith("hdr ") else 1.0)  # BC6H's planes go above 1
    if data.endswith("random"):
        return [rng.random((N, N), dtype=np.float32) * scale for _ in range(ch)]
    return [np.full((N, N), (0.4 + 0.1 * c) * scale, np.float32) for c in range(ch)]  # resident planes of one value each


def case_bytes(ch, kind, fmt):
    if kind == "u8":
        return 4 * ch * PX + 4 * PX
    if kind == "pt":
        return 4 * 4 * PX + (N // 4) * (N // 4) * 8  # alpha is read too
    return 4 * (1 if ch == 1 else PLANES[fmt]) * PX + (N // 4) * (N // 4) * BLOCK_BYTES[fmt]  # decode writes what encode reads


def run(reps):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bc_ref
    kc.init(0)
    imgs = {}
    for ch in (1, 4):
        for data in ("random", "uniform") + (OWN + CUTOUTS if ch == 4 else ()):
            imgs[ch, data] = kc.SlotImage.from_planes(planes_for(ch, data)).materialize()
    own = {data: imgs[4, data].to_bc_torch(BC6H) for data in OWN}
    outs = {f: torch.empty((N // 4, N // 4, BLOCK_BYTES[f]), dtype=torch.uint8, device="cuda") for f in BLOCK_BYTES}
    u8 = torch.empty((N, N, 4), dtype=torch.uint8, device="cuda")
    kc.sync()
    torch.cuda.synchronize()
    for name, ch, data, kind, fmt, srgb in CASES:
        img = imgs[ch, data]
        if kind == "u8":
            call = lambda: img.to_torch(out=u8)  # noqa: E731
        elif kind == "decode":
            call = lambda: kc.SlotImage.from_bc_torch(own[data], N, N, fmt)  # noqa: E731
        elif kind == "compare":
            call = lambda: img.bc_error(fmt, blocks=own[data])  # noqa: E731
        elif kind == "pt":
            call = lambda: img.to_bc_torch(fmt, srgb, out=outs[fmt], punch_through=PT_REF)  # noqa: E731
        else:
            call = lambda: img.to_bc_torch(fmt, srgb, out=outs[fmt])  # noqa: E731
        call()  # warm-up
        torch.cuda.synchronize()
        b0 = kc.stats()["algorithmic_bytes"]
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        print("bytes %-28s %d per call" % (name, (kc.stats()["algorithmic_bytes"] - b0) // reps))
    # the same blocks through the host: kc_image_to_u8 + the numpy reference encoder
    img = imgs[4, "random"]
    for fmt in (1, 3):
        dev_ms, host_ms = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            a = img.to_bc(fmt)
            dev_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()  # once: the numpy encoder takes seconds
        b = bc_ref.encode(img.to_u8(), fmt)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(a, b)
        print("wall RGBA BC%d kc_image_to_bc:                 median %.2f ms" % (fmt, statistics.median(dev_ms)))
        print("wall RGBA BC%d kc_image_to_u8 + numpy encoder: median %.2f ms" % (fmt, statistics.median(host_ms)))
    print("reps %d" % reps)


def report(trace_csv, log):
    lines = open(log).read().splitlines()
    reps = int(next(x.split()[1] for x in lines if x.startswith("reps ")))
    rows = list(csv.DictReader(open(trace_csv)))
    col = lambda key: next(k for k in rows[0] if key in k)  # noqa: E731
    kn, ks, ke = col("Kernel_Name"), col("Start_Timestamp"), col("End_Timestamp")
    rows.sort(key=lambda r: int(r[ks]))
    names = ("bc_encode_kernel", "bc1a_encode_kernel", "bc7_encode_kernel", "bc6h_encode_kernel", "bc6h_decode_kernel", "bc6h_compare_kernel", "image_export_kernel")
    ours = [r for r in rows if any(n in r[kn] for n in names)]
    ours = ours[len(OWN):]
    per = reps + 1
    # the cases' dispatches come first; the wall-clock comparison's calls follow them
    assert len(ours) >= len(CASES) * per, (len(ours), len(CASES) * per)
    out = ["Block compression, %d x %d, MI355X; kernel times from rocprofv3 --kernel-trace (median of %d calls after a warm-up), "
           "fraction of %.0f TB/s = algorithmic bytes (planes read + blocks or pixels written) / time / peak" % (N, N, reps, PEAK_TBS),
           ""]
    out.append("%-30s %10s %10s %9s" % ("case", "median us", "alg MB", "of 8TB/s"))
    for i, (name, ch, _, kind, fmt, _) in enumerate(CASES):
        seg = ours[i * per:(i + 1) * per]
        want = KERNEL.get(kind) or ("bc7_encode_kernel" if fmt == BC7 else "bc6h_encode_kernel" if fmt == BC6H else "bc_encode_kernel")
        assert all(want in r[kn] for r in seg), name
        ns = statistics.median([int(r[ke]) - int(r[ks]) for r in seg[1:]])
        b = case_bytes(ch, kind, fmt)
        out.append("%-30s %10.1f %10.1f %9.3f" % (name, ns / 1e3, b / 1e6, b / ns / 1e3 / PEAK_TBS))
    out.append("")
    out.append("Algorithmic bytes per call (kc_stats_algorithmic_bytes) and wall-clock (a run of its own, without the tracer):")
    out += ["  " + x.rstrip() for x in lines if x.startswith(("bytes ", "wall "))]
    print("\n".join(out))


# ------------------------------------------------------------------ every mode against the single-subset decoders
# (name, fmt, kind, blocks "own" | "every mode", all_modes): the two forms of a case follow one another
MODE_CASES = [("%s %s, %s blocks, %s" % (_kind, "BC7" if _fmt == BC7 else "BC6H", _blocks, "all modes" if _all else "default"), _fmt, _kind, _blocks, _all)
              for _fmt in (BC7, BC6H) for _kind in ("decode", "compare") for _blocks in ("own", "every mode") for _all in (False, True)]
MODE_KERNELS = ("bc_decode_kernel", "bc6h_decode_kernel", "bc7_modes_decode_kernel", "bc6h_modes_decode_kernel", "bc_compare_kernel",
                "bc6h_compare_kernel", "bc7_modes_compare_kernel", "bc6h_modes_compare_kernel")


def modes_kernel(fmt, kind, all_modes):
    if all_modes:
        return "%s_modes_%s_kernel" % ("bc7" if fmt == BC7 else "bc6h", kind)
    return "%s_%s_kernel" % ("bc" if fmt == BC7 else "bc6h", kind)


def modes_run(reps):
    import torch

    import kanter_core_amd as kc
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bc_modes_ref
    kc.init(0)
    imgs = {BC7: kc.SlotImage.from_planes(planes_for(4, "random")).materialize(), BC6H: kc.SlotImage.from_planes(planes_for(4, "hdr random")).materialize()}
    blocks = {}
    for fmt in (BC7, BC6H):
        blocks[fmt, "own"] = imgs[fmt].to_bc_torch(fmt)
        blocks[fmt, "every mode"] = torch.from_numpy(bc_modes_ref.random_image_blocks(fmt, N, N)).cuda()
    kc.sync()
    torch.cuda.synchronize()
    for name, fmt, kind, which, all_modes in MODE_CASES:
        blk = blocks[fmt, which]
        if kind == "decode":
            call = lambda: kc.SlotImage.from_bc_torch(blk, N, N, fmt, all_modes=all_modes)  # noqa: E731
        else:
            call = lambda: imgs[fmt].bc_error(fmt, blocks=blk, all_modes=all_modes)  # noqa: E731
        call()  # warm-up
        torch.cuda.synchronize()
        b0 = kc.stats()["algorithmic_bytes"]
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        kc.sync()
        print("bytes %-50s %d per call" % (name, (kc.stats()["algorithmic_bytes"] - b0) // reps))
    print("reps %d" % reps)


def modes_report(trace_csv, log):
    lines = open(log).read().splitlines()
    reps = int(next(x.split()[1] for x in lines if x.startswith("reps ")))
    rows = list(csv.DictReader(open(trace_csv)))
    col = lambda key: next(k for k in rows[0] if key in k)  # noqa: E731
    kn, ks, ke = col("Kernel_Name"), col("Start_Timestamp"), col("End_Timestamp")
    rows.sort(key=lambda r: int(r[ks]))
    ours = [r for r in rows if any(n + "<" in r[kn] or n + "I" in r[kn] for n in MODE_KERNELS)]
    per = reps + 1
    assert len(ours) == len(MODE_CASES) * per, (len(ours), len(MODE_CASES) * per)
    out = ["Every mode against the single-subset decoders (KC_BC_ALL_MODES), %d x %d, MI355X, one session, the forms alternating; kernel times "
           "from rocprofv3 --kernel-trace (median of %d calls after a warm-up), fraction of %.0f TB/s as above; the compare rows are the "
           "comparison kernel alone" % (N, N, reps, PEAK_TBS), ""]
    out.append("%-52s %10s %10s %9s" % ("case", "median us", "alg MB", "of 8TB/s"))
    for i, (name, fmt, kind, _, all_modes) in enumerate(MODE_CASES):
        seg = ours[i * per:(i + 1) * per]
        assert all(modes_kernel(fmt, kind, all_modes) in r[kn] for r in seg), (name, [r[kn][:40] for r in seg])
        ns = statistics.median([int(r[ke]) - int(r[ks]) for r in seg[1:]])
        b = case_bytes(4, kind, fmt)
        out.append("%-52s %10.1f %10.1f %9.3f" % (name, ns / 1e3, b / 1e6, b / ns / 1e3 / PEAK_TBS))
    out.append("")
    out += ["  " + x.rstrip() for x in lines if x.startswith("bytes ")]
    print("\n".join(out))


if __name__ == "__main__":
    if sys.argv[1] == "modes-run":
        modes_run(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    elif sys.argv[1] == "modes-report":
        modes_report(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        report(sys.argv[2], sys.argv[3])
