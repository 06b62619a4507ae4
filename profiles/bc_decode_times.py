"""Block decode and compare at 4096^2 (csrc/bc_decode.hip): kernel time, algorithmic bytes and the fraction of 8 TB/s per case --
decode of BC1, BC3, BC4, BC5 and BC7 blocks (the library's own encoding of the image) with kc_image_from_device U8 interleaved
beside it, which writes the same four planes; compare of every format (sRGB where it is allowed) with kc_image_to_bc_device of
the same format beside it, which reads the same planes; random data and a uniform image.

    python profiles/bc_decode_times.py run [reps]          (on the GPU box; bytes per call)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/bc_decode_times.py run [reps]
    python profiles/bc_decode_times.py report DIR/.../*_kernel_trace.csv run.log    -> the table (bc_decode_times.txt)

The cases run in a fixed order, each as one warm-up call and `reps` timed calls, so the report assigns the trace's dispatches to
the cases by their order (the encoder launches that make the blocks come first and are skipped).
"""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4096
PEAK_TBS = 8.0
PX = N * N
BC7 = 98  # KC_BC7
BLOCK_BYTES = {1: 8, 3: 16, 4: 8, 5: 16, BC7: 16}
WRITTEN = {1: 4, 3: 4, 4: 1, 5: 2, BC7: 4}  # resident planes a decode writes
READ = {1: 3, 3: 4, 4: 1, 5: 2, BC7: 4}     # planes a compare (and the encoder) reads
FORMS = ((1, False), (1, True), (3, False), (3, True), (4, False), (5, False), (BC7, False), (BC7, True))
KERNEL = {"decode": "bc_decode_kernel", "import": "image_import_kernel", "compare": "bc_compare_kernel", "encode": "_encode_kernel"}


def bc_name(fmt, srgb=False):
    return "BC%d%s" % (7 if fmt == BC7 else fmt, " sRGB" if srgb else "")


# (name, data, kind, fmt, srgb)
CASES = []
for _data in ("random", "uniform"):
    for _fmt in (1, 3, 4, 5, BC7):
        CASES.append(("decode %s %s" % (bc_name(_fmt), _data), _data, "decode", _fmt, False))
    CASES.append(("from_device U8 RGBA %s" % _data, _data, "import", 0, False))
    for _fmt, _srgb in FORMS:
        CASES.append(("compare %s %s" % (bc_name(_fmt, _srgb), _data), _data, "compare", _fmt, _srgb))
        CASES.append(("to_bc %s %s" % (bc_name(_fmt, _srgb), _data), _data, "encode", _fmt, _srgb))


def case_bytes(kind, fmt):
    blocks = (N // 4) * (N // 4) * BLOCK_BYTES.get(fmt, 0)
    if kind == "import":
        return 4 * PX + 4 * 4 * PX
    if kind == "decode":
        return blocks + 4 * WRITTEN[fmt] * PX
    return 4 * READ[fmt] * PX + blocks


def run(reps):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    rng = np.random.default_rng(4)
    imgs = {"random": kc.SlotImage.from_planes([rng.random((N, N), dtype=np.float32) for _ in range(4)]).materialize(),
            "uniform": kc.SlotImage.from_planes([np.full((N, N), 0.4 + 0.1 * c, np.float32) for c in range(4)]).materialize()}
    blocks = {(d, f, s): imgs[d].to_bc_torch(f, s) for d in imgs for f, s in FORMS}
    u8 = {d: imgs[d].to_torch(dtype=torch.uint8) for d in imgs}
    out = {f: torch.empty((N // 4, N // 4, BLOCK_BYTES[f]), dtype=torch.uint8, device="cuda") for f in BLOCK_BYTES}
    kc.sync()
    torch.cuda.synchronize()
    print("setup %d" % len(blocks))
    for name, data, kind, fmt, srgb in CASES:
        img = imgs[data]
        call = {"decode": lambda: kc.SlotImage.from_bc_torch(blocks[data, fmt, False], N, N, fmt),
                "import": lambda: kc.SlotImage.from_torch(u8[data]),
                "compare": lambda: img.bc_error(fmt, srgb, blocks=blocks[data, fmt, srgb]),
                "encode": lambda: img.to_bc_torch(fmt, srgb, out=out[fmt])}[kind]
        call()  # warm-up
        torch.cuda.synchronize()
        b0 = kc.stats()["algorithmic_bytes"]
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        kc.sync()
        print("bytes %-30s %d per call" % (name, (kc.stats()["algorithmic_bytes"] - b0) // reps))
    e1, e7 = imgs["random"].bc_error(1), imgs["random"].bc_error(BC7)
    print("psnr random RGB: BC1 %.2f dB, BC7 %.2f dB" % (e1.psnr(), e7.psnr(channels=(0, 1, 2))))
    print("reps %d" % reps)


def report(trace_csv, log):
    lines = open(log).read().splitlines()
    reps = int(next(x.split()[1] for x in lines if x.startswith("reps ")))
    setup = int(next(x.split()[1] for x in lines if x.startswith("setup ")))
    rows = list(csv.DictReader(open(trace_csv)))
    col = lambda key: next(k for k in rows[0] if key in k)  # noqa: E731
    kn, ks, ke = col("Kernel_Name"), col("Start_Timestamp"), col("End_Timestamp")
    rows.sort(key=lambda r: int(r[ks]))
    ours = [r for r in rows if any(k in r[kn] for k in KERNEL.values())]
    enc = [i for i, r in enumerate(ours) if KERNEL["encode"] in r[kn]]
    ours = ours[enc[setup - 1] + 1:]  # the encoder launches that made the blocks
    ours = [r for r in ours if "image_export_kernel" not in r[kn]]
    per = reps + 1
    assert len(ours) >= len(CASES) * per, (len(ours), len(CASES) * per)
    out = ["Block decode and compare, %d x %d, MI355X; kernel times from rocprofv3 --kernel-trace (median of %d calls after a warm-up), "
           "fraction of %.0f TB/s = algorithmic bytes (blocks + planes written, or planes read + blocks) / time / peak; the compare rows are "
           "the comparison kernel alone, its combining launch is the last row" % (N, N, reps, PEAK_TBS), ""]
    out.append("%-32s %10s %10s %9s" % ("case", "median us", "alg MB", "of 8TB/s"))
    for i, (name, _, kind, fmt, _) in enumerate(CASES):
        seg = ours[i * per:(i + 1) * per]
        assert all(KERNEL[kind] in r[kn] for r in seg), (name, [r[kn][:40] for r in seg])
        ns = statistics.median([int(r[ke]) - int(r[ks]) for r in seg[1:]])
        b = case_bytes(kind, fmt)
        out.append("%-32s %10.1f %10.1f %9.3f" % (name, ns / 1e3, b / 1e6, b / ns / 1e3 / PEAK_TBS))
    comb = [int(r[ke]) - int(r[ks]) for r in rows if "bc_combine_kernel" in r[kn]]
    if comb:
        out.append("%-32s %10.1f" % ("bc_combine_kernel (%d calls)" % len(comb), statistics.median(comb) / 1e3))
    out.append("")
    out.append("Algorithmic bytes per call (kc_stats_algorithmic_bytes):")
    out += ["  " + x.rstrip() for x in lines if x.startswith(("bytes ", "psnr "))]
    print("\n".join(out))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        report(sys.argv[2], sys.argv[3])
