"""Mip chains at 4096^2 (csrc/mip.hip): the whole chain of one image in three forms --
    (a) kc_image_build_mips, the fused pyramid kernel (two launches),
    (b) the same with KC_MIP_PER_LEVEL (twelve launches of the one-level kernel),
    (c) what the library offered before: kc_resize_image with Triangle from each level to the next one's size, materialised
        (the bits differ: a filtered minification; the job is the same)
-- for an RGBA image with a constant alpha, a Gray image and an RGBA image of four resident planes.  The forms alternate;
then a normal map -- a kc_height_to_normal_process result, three resident planes and a constant alpha -- as mips() against
mips(normals=True) (csrc/mip_normals.hip: the same bytes moved, every level renormalised), alternating in the same way;
every round times CALLS calls back to back between two HIP events on the library's stream (profiler off) and reports us per
call, so a figure holds the host's share of a call wherever the host is the slower side; the host's own time per call is
printed beside it.  Also: (a) == (b) byte for byte at 4096^2 and 8192 x 2048, and the wall-clock of to_bc_mips against to_bc.

    python profiles/mip_times.py [rounds] [calls]          (on the GPU box)        -> profiles/mip_times.txt
    python profiles/mip_times.py [rounds] [calls] normals  the normal-map case alone
    KC_LIB_PATH=profiles/ab_libs/NAME.so python profiles/mip_times.py ...       another build of the library, for A/B runs (section 2
                                                                                 of mip_times.txt: a build variant of mip.hip that is
                                                                                 no longer kept)
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4096
PEAK_TBS = 8.0


def level_sizes(w, h):
    return [(max(1, w >> k), max(1, h >> k)) for k in range(max(w, h).bit_length())]


def normals_case(kc, np, timed, rounds):
    """mips() against mips(normals=True) on a HeightToNormal result: both read three planes and write three per level"""
    rng = np.random.default_rng(4097)
    img = kc.height_to_normal_process(kc.SlotImage.from_planes([rng.random((N, N), dtype=np.float32)]))
    forms = [("plain", lambda i: i.mips()), ("normals", lambda i: i.mips(normals=True)),
             ("normals, per level", lambda i: i.mips(per_level=True, normals=True))]
    for _, fn in forms:
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
    img.mips(normals=True)
    l1 = kc.stats()
    alg = l1["algorithmic_bytes"] - l0["algorithmic_bytes"]
    print("Normal map: kc_height_to_normal_process of a %d x %d height (3 resident planes, constant alpha; normals: %d launches, %.1f MB algorithmic)"
          % (N, N, l1["kernel_launches"] - l0["kernel_launches"], alg / 1e6))
    for f, _ in forms:
        r = runs[f]
        print("  %-20s %s   range %.1f - %.1f   median %.1f   host median %.1f" % (
            f, " ".join("%7.1f" % x for x in r), min(r), max(r), statistics.median(r), statistics.median(hosts[f])))
    a, b = runs["plain"], runs["normals"]
    print("  normals - plain, medians: %.1f us;  normals by algorithmic bytes: %.3f of %.0f TB/s" % (
        statistics.median(b) - statistics.median(a), alg / (statistics.median(b) * 1e-6) / 1e12 / PEAK_TBS, PEAK_TBS))
    fused, per_level = img.mips(normals=True), img.mips(per_level=True, normals=True)
    for k, (x, y) in enumerate(zip(fused, per_level)):
        for p, q in zip(x.planes(), y.planes()):
            assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), k
    worst = 0.0
    for lv in fused[1:]:
        d = np.stack(lv.planes()[:3]).astype(np.float64) * 2.0 - 1.0
        worst = max(worst, float(np.abs(np.sqrt((d * d).sum(axis=0)) - 1.0).max()))
    short = min(float(np.sqrt(((np.stack(lv.planes()[:3]).astype(np.float64) * 2.0 - 1.0) ** 2).sum(axis=0)).min()) for lv in img.mips()[1:])
    print("  normals: fused == per level byte for byte, %d levels; max | |v| - 1 | over levels >= 1: %.2g (plain: shortest vector %.3f)"
          % (len(fused), worst, short))
    print()


def main(rounds, calls, only_normals=False):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    lib_stream = torch.cuda.ExternalStream(kc.get_stream(), device=torch.device("cuda", 0))

    def timed(fn, img):
        """us per call on the device's clock and on the host's"""
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

    print("Mip chains of a %d x %d image, MI355X, library %s" % (N, N, os.environ.get("KC_LIB_PATH", "as built")))
    print("%d rounds, the forms alternating; each figure: %d calls back to back between two HIP events on the library's stream,"
          % (rounds, calls))
    print("us per call (profiler off); host = the host's own time per call in the same window")
    print()
    if only_normals:
        normals_case(kc, np, timed, rounds)
        return
    rng = np.random.default_rng(4096)
    plane = lambda w=N, h=N: rng.random((h, w), dtype=np.float32)  # noqa: E731
    rgb = [kc.SlotImage.from_planes([plane()]) for _ in range(3)]
    const_alpha = lambda: kc.combine_rgba_process(rgb + [kc.SlotImage.from_value(kc.Size(N, N), 0.5, False)])  # noqa: E731
    gray, rgba = kc.SlotImage.from_planes([plane()]), kc.SlotImage.from_planes([plane() for _ in range(4)])
    # (image for (a) and (b), image for (c), resident planes): kc_resize_image fills a constant plane of its source in place, so
    # (c) gets a constant-alpha image of its own (the same R, G, B planes) and (a), (b) keep theirs constant
    images = {"RGBA, constant alpha": (const_alpha(), const_alpha(), 3), "Gray": (gray, gray, 1), "RGBA, four planes": (rgba, rgba, 4)}
    sizes = level_sizes(N, N)

    def resize_chain(img):
        out = [img]
        for w, h in sizes[1:]:
            out.append(kc.resize_image(out[-1], kc.Size(w, h), kc.ResizeFilter.Triangle).materialize())
        return out

    forms = [("(a) fused", lambda img: img.mips()), ("(b) per level", lambda img: img.mips(per_level=True)),
             ("(c) resize loop", resize_chain)]

    medians = {}
    for name, (img, img_c, n_res) in images.items():
        of = lambda f: img_c if f.startswith("(c)") else img  # noqa: E731
        for f, fn in forms:  # warm-up: code objects, tap tables, pool blocks
            fn(of(f))
            fn(of(f))
        kc.sync()
        runs = {f: [] for f, _ in forms}
        hosts = {f: [] for f, _ in forms}
        for _ in range(rounds):
            for f, fn in forms:
                dev, host = timed(fn, of(f))
                runs[f].append(dev)
                hosts[f].append(host)
        l0 = kc.stats()
        img.mips()
        l1 = kc.stats()
        alg = l1["algorithmic_bytes"] - l0["algorithmic_bytes"]
        print("%s (%d resident planes; (a): %d launches, %.1f MB algorithmic)" % (name, n_res, l1["kernel_launches"] - l0["kernel_launches"],
                                                                                   alg / 1e6))
        for f, _ in forms:
            r = runs[f]
            medians[name, f] = statistics.median(r)
            print("  %-16s %s   range %.1f - %.1f   median %.1f   host median %.1f" % (
                f, " ".join("%7.1f" % x for x in r), min(r), max(r), statistics.median(r), statistics.median(hosts[f])))
        a, b, c = (runs[f] for f, _ in forms)
        print("  (a) wholly below (c): %s;  (a) / (b) medians %.2f;  (a) by algorithmic bytes: %.3f of %.0f TB/s" % (
            "yes" if max(a) < min(c) else "NO", statistics.median(a) / statistics.median(b),
            alg / (statistics.median(a) * 1e-6) / 1e12 / PEAK_TBS, PEAK_TBS))
        print()

    normals_case(kc, np, timed, rounds)

    # (a) == (b), byte for byte, at full size
    for w, h in ((N, N), (8192, 2048)):
        img = kc.SlotImage.from_planes([plane(w, h) for _ in range(4)])
        fused, per_level = img.mips(), img.mips(per_level=True)
        assert len(fused) == len(per_level) == len(level_sizes(w, h))
        for k, (x, y) in enumerate(zip(fused, per_level)):
            assert tuple(x.size()) == tuple(y.size()) == level_sizes(w, h)[k]
            for p, q in zip(x.planes(), y.planes()):
                assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), (w, h, k)
        print("(a) == (b) byte for byte at %d x %d, RGBA, %d levels" % (w, h, len(fused)))
        del img, fused, per_level
    print()

    # the BC chain against level 0 alone, wall-clock of the blocking host forms (encode + copy to host memory)
    img = rgba
    for fmt in (1, 3):
        one, chain = [], []
        for _ in range(7):
            t0 = time.perf_counter()
            img.to_bc(fmt)
            one.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            img.to_bc_mips(fmt)
            chain.append((time.perf_counter() - t0) * 1e3)
        print("wall BC%d: to_bc (level 0) median %.2f ms (%.2f - %.2f);  to_bc_mips (13 levels) median %.2f ms (%.2f - %.2f)" % (
            fmt, statistics.median(one), min(one), max(one), statistics.median(chain), min(chain), max(chain)))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 20, sys.argv[3:] == ["normals"])
