"""The option table (csrc/c_api.cpp): kc_set_option / kc_get_option, the three dedicated setters and the KC_<NAME> environment
variables that kc_init reads.  No GPU needed: every case runs in a fresh child process that never initialises a device, or
whose kc_init fails on validation before its first HIP call."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 102

# name: (default, accepted samples, refused samples).  A flag stores any integer as 0 / 1.
FLAG = "flag"
OPTIONS = {
    "chain1": (1, FLAG, []),
    "replay": (1, FLAG, []),
    "join": (1, FLAG, []),
    "wide": (1, FLAG, []),
    "fusion": (1, FLAG, []),
    "down2": (1, [0, 1, 2], [-1, 3, 5]),
    "down2_by_rows": (-1, [-1, 0, 1], [-2, 2]),
    "poly2": (1, [0, 1], [-1, 2]),
    "poly2_min_ratio": (8, [2, 4, 1000], [1, 0, -8]),
    "resize_mode": (0, [0, 1, 2, 3, 4], [-1, 5]),
    "resize_tile_w": (0, [0, 4, 64, 1024], [-1, 1025]),
    "resize_tile_h": (0, [0, 8, 32, 64], [-1, 65]),
    "poly_rows": (0, [0, 4, 8, 24], [-1]),
    "poly2_xcd": (-1, [-1, 0, 1, 2], [-2, 3]),
    "down2_xcd": (-1, [-1, 0, 1], [-2, 2]),
    "h2n_tiled": (-1, [-1, 0, 1], [-2, 2]),
    "cache_policy": (1, [0, 1], [-1, 2]),
    "cache_budget_mb": (208, [0, 1, 4096], [-1]),
    "nt_force": (-1, [-1, 0, 0x100, 0x1ff], [-2]),
    "chain_unroll": (0, [0, 1, 2, 4, 6, 8], [-1, 3, 5, 7, 9, 16]),
    "max_blocks": (4096, [1, 65536], [0, -1]),
    "tune_cap": (0, [0, 8192], [-1]),
    "upload_ring": (1, FLAG, []),
    "link_gbps": (153, [1, 600], [0, -1]),
    "hbm_gbps": (6100, [1, 8000], [0, -1]),
}
FLAG_SAMPLES = [0, 1, 7, -3, 0]
DEDICATED = {"fusion": "kc_%s_fusion", "resize_mode": "kc_%s_resize_mode", "cache_policy": "kc_%s_cache_policy"}
# the environment variables read outside the option table, each for a reason of its own
OWN_GETENV = {"KC_SPEC_WG", "KC_SPECIALIZE", "KC_KERNEL_CACHE_DIR", "KC_KERNEL_CACHE_MANIFEST", "XDG_CACHE_HOME", "HOME",
              "KC_COMM_TRANSPORT", "KC_COMM_TIMEOUT_S", "KC_SAMPLE_OUT"}


def env_name(name):
    return "KC_" + name.upper()


def run_child(code, **env):
    """Runs `code` in a fresh interpreter with the library importable and no option variable set but `env`; returns the JSON
    the code prints last."""
    e = {k: v for k, v in os.environ.items() if k not in {env_name(n) for n in OPTIONS}}
    e.update(env)
    prelude = "import ctypes as C, json, os\nfrom kanter_core_amd import _lib\nL = _lib.load()\n"
    r = subprocess.run([sys.executable, "-c", prelude + code], cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


GET = """
def get(name):
    v = C.c_int(-12345)
    s = L.kc_get_option(name.encode(), C.byref(v))
    return [s, v.value]
"""


@pytest.fixture(scope="module")
def round_trips():
    """Per name: the default, then (value, status, value read back, last error) for every accepted and refused sample."""
    code = GET + """
out = {}
for name, (dflt, ok, bad) in json.loads(os.environ["KC_TEST_OPTIONS"]).items():
    rec = {"default": get(name), "ok": [], "bad": []}
    for v in (%r if ok == "flag" else ok):
        rec["ok"].append([v, L.kc_set_option(name.encode(), v), get(name)[1]])
    for v in bad:
        s = L.kc_set_option(name.encode(), v)
        rec["bad"].append([v, s, get(name)[1], L.kc_last_error().decode()])
    out[name] = rec
print(json.dumps(out))
""" % (FLAG_SAMPLES,)
    return run_child(code, KC_TEST_OPTIONS=json.dumps(OPTIONS))


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_default_before_init(round_trips, name):
    assert round_trips[name]["default"] == [0, OPTIONS[name][0]]


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_accepted_values_round_trip(round_trips, name):
    flag = OPTIONS[name][1] == FLAG
    for v, status, back in round_trips[name]["ok"]:
        assert status == 0, (name, v)
        assert back == ((1 if v else 0) if flag else v), (name, v)


@pytest.mark.parametrize("name", sorted(n for n in OPTIONS if OPTIONS[n][2]))
def test_refused_values_leave_the_option_alone(round_trips, name):
    last_ok = round_trips[name]["ok"][-1][2]
    for v, status, back, err in round_trips[name]["bad"]:
        assert status == INVALID_ARG, (name, v)
        assert back == last_ok, (name, v)
        assert name in err and "accepts" in err and "unknown" not in err, err


def test_unknown_names_are_refused():
    res = run_child(GET + """
print(json.dumps([L.kc_set_option(b"no_such_option", 1), get("no_such_option")[0], L.kc_get_option(b"", C.byref(C.c_int())),
                  L.kc_set_option(b"KC_DOWN2", 1), L.kc_last_error().decode()]))
""")
    assert res[:4] == [INVALID_ARG] * 4
    assert "unknown option KC_DOWN2" in res[4]


@pytest.mark.parametrize("name", sorted(DEDICATED))
def test_dedicated_setters_are_the_same_option(name):
    set_fn, get_fn = DEDICATED[name] % "set", DEDICATED[name] % "get"
    res = run_child(GET + """
out = []
for v in (3, 0, 1, 5, -1, 7):
    s = L.%s(v)
    out.append([v, s, get("%s")[1], L.%s()])
for v in (0, 1):
    L.kc_set_option(b"%s", v)
    out.append([v, 0, get("%s")[1], L.%s()])
print(json.dumps(out))
""" % (set_fn, name, get_fn, name, name, get_fn))
    prev = OPTIONS[name][0]
    for v, status, via_option, via_getter in res:
        assert via_option == via_getter, (name, v)
        if OPTIONS[name][1] == FLAG:  # kc_set_fusion takes any integer
            assert status == 0 and via_option == (1 if v else 0), (name, v)
        elif v in OPTIONS[name][1]:
            assert status == 0 and via_option == v, (name, v)
        else:
            assert status == INVALID_ARG and via_option == prev, (name, v)
        prev = via_option


INIT = GET + """
import kanter_core_amd as kc
try:
    kc.init(0)
    err = None
except kc.TexProError as e:
    err = [e.code, str(e)]
print(json.dumps({"err": err, "down2": get("down2")[1], "chain_unroll": get("chain_unroll")[1], "replay": get("replay")[1],
                  "init": L.kc_is_initialized()}))
"""


@pytest.mark.parametrize("var, value", [
    ("KC_DOWN2", "7"),            # a range
    ("KC_CHAIN_UNROLL", "3"),     # a set
    ("KC_REPLAY", "off"),         # a flag: any integer, but an integer
    ("KC_MAX_BLOCKS", "0"),
    ("KC_POLY2", "2"),
    ("KC_DOWN2", "1.5"),
    ("KC_DOWN2", "0x1"),          # decimal only (but KC_NT_FORCE, below)
    ("KC_DOWN2", ""),
    ("KC_CACHE_BUDGET_MB", "-1"),
    ("KC_POLY_ROWS", "99999999999"),
])
def test_refused_environment_fails_init(var, value):
    res = run_child(INIT, **{var: value})
    assert res["err"] is not None and res["err"][0] == INVALID_ARG, res
    assert "%s=%s refused" % (var, value) in res["err"][1], res
    assert res["init"] == 0
    assert (res["down2"], res["chain_unroll"], res["replay"]) == (1, 0, 1)  # nothing committed


def test_one_refused_variable_commits_none():
    # KC_NT_FORCE=0x100 passes (a mask: any base), KC_DOWN2=2 passes, KC_CHAIN_UNROLL=3 does not: nothing is committed
    res = run_child(INIT, KC_NT_FORCE="0x100", KC_DOWN2="2", KC_CHAIN_UNROLL="3")
    assert res["err"][0] == INVALID_ARG and "KC_CHAIN_UNROLL=3 refused" in res["err"][1], res
    assert (res["down2"], res["chain_unroll"]) == (1, 0)


def _csrc_sources():
    d = os.path.join(ROOT, "kanter_core_amd", "csrc")
    for fn in sorted(os.listdir(d)):
        p = os.path.join(d, fn)
        if os.path.isfile(p):
            with open(p) as f:
                yield fn, f.read()


def test_getenv_only_in_the_option_table_and_for_its_exceptions():
    literal, other = set(), []
    for fn, text in _csrc_sources():
        for m in re.finditer(r'getenv\(\s*(?:"([^"]*)"|(\w+))', text):
            if m.group(1) is not None:
                literal.add(m.group(1))
            else:
                other.append((fn, m.group(2)))
    assert literal <= OWN_GETENV, sorted(literal - OWN_GETENV)
    assert other == [("c_api.cpp", "var")], other  # options_from_env: KC_<NAME> of every row


def test_table_matches_the_test_and_the_header_list():
    with open(os.path.join(ROOT, "kanter_core_amd", "csrc", "c_api.cpp")) as f:
        src = f.read()
    table = src[src.index("constexpr OptionRow kOptions[]"):]
    table = table[:table.index("};")]
    names = re.findall(r'KC_(?:FLAG|RANGE)\((\w+)|"(\w+)"', table)
    names = [a or b for a, b in names]
    assert sorted(names) == sorted(OPTIONS) and len(names) == len(set(names))
    with open(os.path.join(ROOT, "include", "kanter_core_amd.h")) as f:
        hdr = f.read()
    end = hdr.index("KC_API int kc_set_option(")
    doc = hdr[hdr.rindex("/*", 0, end):end]
    for n in names:
        assert doc.count('"%s"' % n) == 1, n
