"""The counters of the streaming kernels' launch variants (tests/test_gpu_streaming_variants.py reads them on the device): every
name is listed at kc_stats_counter in the header and counted by the host code, under exactly that spelling."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["h2n_launches", "h2n_plain", "h2n_tiled_q5", "h2n_tiled_q6", "h2n_tiled_q7", "h2n_band", "h2n_nt", "to_u8_nt", "from_u8_nt",
         "image_import_vec", "image_import_scalar", "image_import_nt", "image_export_vec", "image_export_scalar", "image_export_nt",
         "stats_nt", "mip_nt"]


def test_header_lists_and_host_counts_every_streaming_counter():
    header = open(os.path.join(ROOT, "include", "kanter_core_amd.h")).read()
    comment = header[:header.index("KC_API int kc_stats_counter")].rsplit("/*", 1)[1]
    host = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "kanter_core_amd", "csrc", "*.cpp")))
    counted = set(re.findall(r'"([a-z0-9_]+)"', "".join(re.findall(r"c\.counters\[([^\]]*)\]", host))))
    for name in NAMES:
        assert '"%s"' % name in comment, name
        assert name in counted, name
