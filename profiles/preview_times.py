"""Previews (csrc/preview.hip, kc_image_previews) against the only route the library had before, per image: kc_image_build_mips
(the whole chain, every level written) + to_u8 of the level + the copy.  Cases:
    (1) 32 RGBA 1024^2 images at the level preview_level(1024, 1024, 128) names, as ONE batch -- an editor's thumbnails;
    (2) one 4096^2 RGBA image at level 5 (128 x 128);
    (3) a 512 x 512 rect of level 0, and of level 1, of a 4096^2 RGBA image -- a viewport.
The two routes alternate in one session, profiler off.  Per case: wall clock per batch of the blocking host forms, device time
of the device forms through the C ABI, arguments built beforehand (CALLS calls back to back between two HIP events on the
library's stream: a figure holds the host's share of a call wherever the host is the slower side), launches and algorithmic bytes
per batch; for (2) the fraction of 8 TB/s by algorithmic bytes, beside mip_pyramid_kernel's (img.mips()) in the same session.

    python profiles/preview_times.py [rounds] [calls]          (on the GPU box)        -> profiles/preview_times.txt
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0


def main(rounds, calls):
    import numpy as np
    import torch

    import kanter_core_amd as kc
    kc.init(0)
    lib_stream = torch.cuda.ExternalStream(kc.get_stream(), device=torch.device("cuda", 0))
    rng = np.random.default_rng(1024)
    image = lambda n: kc.SlotImage.from_planes([rng.random((n, n), dtype=np.float32) for _ in range(4)])  # noqa: E731
    thumbs = [image(1024) for _ in range(32)]
    big = image(4096)
    k_thumb = kc.preview_level(1024, 1024, 128)[0]
    cases = [("(1) 32 x RGBA 1024^2, level %d (128 x 128), one batch" % k_thumb, [(im, k_thumb, None) for im in thumbs]),
             ("(2) RGBA 4096^2, level 5 (128 x 128)", [(big, 5, None)]),
             ("(3a) RGBA 4096^2, level 0, rect 512 x 512 at (1001, 777)", [(big, 0, (1001, 777, 512, 512))]),
             ("(3b) RGBA 4096^2, level 1, rect 512 x 512 at (1001, 777)", [(big, 1, (1001, 777, 512, 512))])]

    def cut(a, rect):
        if rect is None:
            return a
        x, y, w, h = rect
        return a[y:y + h, x:x + w]

    def old_host(reqs):  # per image: the chain, to_u8 of the level, the copy (to_u8 blocks)
        return [cut((im.mips()[k] if k else im).to_u8(), rect) for im, k, rect in reqs]

    def new_host(reqs):
        return kc.previews(reqs)

    # the device forms through the C ABI with arguments built beforehand, on the library's own stream: what a host in C or Rust calls
    from kanter_core_amd import _lib
    from kanter_core_amd.api import _preview_requests, device_image_desc
    L = _lib.load()

    def old_device(reqs, outs):
        for (im, k, rect), (desc, arr, count) in zip(reqs, outs):
            if k == 0:
                L.kc_image_to_device(im._h, C.byref(desc), 0, None)
                continue
            L.kc_image_build_mips(im._h, 0, arr, len(arr), C.byref(count))
            L.kc_image_to_device(arr[k], C.byref(desc), 0, None)
            for j in range(count.value):
                L.kc_image_release(arr[j])

    def new_device(reqs, out):
        arr, n, ptr, nbytes = out
        L.kc_image_previews_device(arr, n, 0, ptr, nbytes, None)

    def wall(fn, reqs):
        kc.sync()
        t0 = time.perf_counter()
        fn(reqs)
        return (time.perf_counter() - t0) * 1e3

    def device(fn, *args):
        kc.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(lib_stream)
        for _ in range(calls):
            fn(*args)
        e1.record(lib_stream)
        e1.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    def counted(fn, *args):
        s0 = kc.stats()
        fn(*args)
        kc.sync()
        s1 = kc.stats()
        return s1["kernel_launches"] - s0["kernel_launches"], s1["algorithmic_bytes"] - s0["algorithmic_bytes"]

    print("Previews against build_mips + to_u8 per image, MI355X, library %s" % os.environ.get("KC_LIB_PATH", "as built"))
    print("%d rounds, the routes alternating.  wall: ms per batch of the blocking host forms (bytes in host memory).  device: us per"
          % rounds)
    print("batch of the device forms, %d calls back to back between two HIP events on the library's stream (profiler off)." % calls)
    print()
    for name, reqs in cases:
        sizes = [((max(1, im.size().width >> k), max(1, im.size().height >> k)) if rect is None else rect[2:]) for im, k, rect in reqs]
        old_t = [torch.empty((max(1, im.size().height >> k), max(1, im.size().width >> k), 4), dtype=torch.uint8, device="cuda") for im, k, _ in reqs]
        new_t = torch.empty((sum(4 * w * h for w, h in sizes),), dtype=torch.uint8, device="cuda")
        old_outs = [(device_image_desc(t, "hwc"), (C.c_void_p * kc.mip_level_count(im.size().width, im.size().height))(), C.c_uint32())
                    for t, (im, _, _) in zip(old_t, reqs)]
        new_out = (_preview_requests([(im._h, im.size(), k, rect) for im, k, rect in reqs])[0], len(reqs), C.c_void_p(new_t.data_ptr()), new_t.numel())
        a, b = old_host(reqs), new_host(reqs)  # warm-up, and the same bytes
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        old_device(reqs, old_outs)
        new_device(reqs, new_out)
        kc.sync()
        assert all(np.array_equal(cut(t.cpu().numpy(), rect), x) for t, (_, _, rect), x in zip(old_t, reqs, a)), name
        at = 0
        for x in b:  # the device form's bytes, tightly packed in request order
            assert np.array_equal(new_t[at:at + x.size].cpu().numpy().reshape(x.shape), x), name
            at += x.size
        w_old, w_new, d_old, d_new = [], [], [], []
        for _ in range(rounds):
            w_old.append(wall(old_host, reqs))
            w_new.append(wall(new_host, reqs))
            d_old.append(device(old_device, reqs, old_outs))
            d_new.append(device(new_device, reqs, new_out))
        l_old, b_old = counted(old_device, reqs, old_outs)
        l_new, b_new = counted(new_device, reqs, new_out)
        print(name)
        for what, w, d, l, by in (("build_mips + to_u8", w_old, d_old, l_old, b_old), ("previews", w_new, d_new, l_new, b_new)):
            print("  %-20s wall ms  median %8.3f (%8.3f - %8.3f)   device us  median %9.1f (%9.1f - %9.1f)   %3d launches  %8.2f MB algorithmic"
                  % (what, statistics.median(w), min(w), max(w), statistics.median(d), min(d), max(d), l, by / 1e6))
        print("  previews / yardstick: wall %.3f, device %.3f;  previews by algorithmic bytes: %.3f of %.0f TB/s" % (
            statistics.median(w_new) / statistics.median(w_old), statistics.median(d_new) / statistics.median(d_old),
            b_new / (statistics.median(d_new) * 1e-6) / 1e12 / PEAK_TBS, PEAK_TBS))
        print()
    # mip_pyramid_kernel on the same image in the same session: the whole chain, two launches
    big.mips()
    d = [device(lambda: big.mips()) for _ in range(rounds)]
    _, by = counted(lambda: big.mips())
    print("RGBA 4096^2, img.mips() (mip_pyramid_kernel, every level written): device us median %.1f (%.1f - %.1f), %.2f MB algorithmic,"
          % (statistics.median(d), min(d), max(d), by / 1e6))
    print("  %.3f of %.0f TB/s" % (by / (statistics.median(d) * 1e-6) / 1e12 / PEAK_TBS, PEAK_TBS))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
