"""GPU parity, differential, of the forms only a LONG-LIVED graph runs: the random graphs of tests/steady_fuzz.py, each built
once and evaluated over and over on the same live graph, every evaluation compared with the oracle (oracle.RefGraph) bit for bit,
NaN == NaN.  The other graph fuzzers (test_gpu_fuzz_graphs.py, _bands, _consumers) evaluate a fresh graph once in the default
mode: a program seen once runs in the step interpreter, so they never reach
  * kernels compiled for a program (csrc/specialize.cpp), the only form that runs joined chains (CH_SAVE_LOAD), programs of 5 to
    16 input planes and two quads per lane ("_q2");
  * the same kernels reading packed copies of long-lived sources (csrc/chain_pack.cpp, U8 and FIX24 tiers, "_pk");
  * the compiled up-sampling chain kernel;
  * replay (csrc/replay.cpp).
Before every evaluation one edge out of every Embed node is plugged in again (connect with the same ends), which dirties
everything below the sources.  Two regimes:
  forced   set_specialize(2), set_pack_sources(2), join and replay on: the first of four evaluations compiles every program and
           packs every eligible source, the later ones record and replay;
  natural  the default modes with cache_budget_mb = 0 (every launch counts as HBM-bound, so pack_sources = 1 packs at the second
           sighting) and specialize_wait() after each of six evaluations: plain chains or join fall-backs first, then compiled
           wide and joined kernels, the pack pass, "_pk" launches, replay.
Each seed has one cache policy (defaults, cache_budget_mb = 0, nt_force = 0x101: the warm form that selects "_q2"); nothing else
is forced.  Pow (one ulp from the oracle, which later nodes amplify) has a sweep of its own, device against device: the forced
regime's last evaluation against one evaluation with everything off; the interpreter and the compiled kernels are bit-identical
on Pow (test_gpu_pow.py).  The kernel cache points at a temporary directory while the module runs.

The last tests hold the coverage: every form's counter rose, for at least 8 different seeds each, and a one-launch program of
more than 8 input planes ran.  Measured on an MI355X when written, the module alone (seeds that raised the counter / its rise):
  join_launches 82 / 366, wide_launches 41 / 178, join_fallbacks 27 / 119, packed_launches 16 / 113, packed_planes 18 / 57,
  pack_rejected 27 / 270, replayed_evaluations 36 / 88, upsample_chain_launches 17 / 189, resize_chain_launches 24 / 221,
  specialized_launches 103 / 1126, "_q2" forms 16 / 186, "_pk" forms 16 / 146; 7 seeds with a one-launch program of 9 or more planes.
hiprtc: 314 kernels compiled; the forced regime's first evaluations took 14.3 s for 130 kernels, 0.11 s each (the process's first
program included, which DESIGN.md puts at about 2 s).  The module takes 34 s, its slowest case 2.3 s (137 cases)."""
import contextlib
import os
import time

import pytest

import steady_fuzz as sf
from util import assert_planes

pytestmark = pytest.mark.gpu

OPTIONS = ("join", "replay", "cache_budget_mb", "nt_force")
COUNTERS = ["join_launches", "wide_launches", "join_fallbacks", "packed_launches", "packed_planes", "pack_rejected",
            "replayed_evaluations", "upsample_chain_launches", "resize_chain_launches"]
# the cache-policy masks the three policies give a compiled kernel: none, nt_force's 0x101, and with a budget of 0 every input
# (inputs 8 to 15 are not part of the name) and the result
_MASKS = [0x000, 0x101] + [0x100 | ((1 << n) - 1) for n in range(1, 9)]
Q2 = ["specialized_nt_%03x_q2%s" % (m, pk) for m in _MASKS for pk in ("", "_pk")]
PK = ["specialized_nt_%03x%s_pk" % (m, q) for m in _MASKS for q in ("", "_q2")]
FLOORS = COUNTERS + ["specialized_launches", "q2", "pk"]

_SAVED = {}
_BASE = {}                        # the counters when the module began
SEEN = {n: set() for n in FLOORS}  # counter -> the seeds whose evaluations raised it
WIDE9 = set()                     # seeds with an evaluation that was ONE launch, wide, over 9 or more distinct source planes
RAN = set()
COMPILE = [0.0, 0]                # seconds in, and kernels compiled by, the forced regime's first evaluations


def _switches(kc):
    return dict(options={n: kc.get_option(n) for n in OPTIONS}, specialize=kc.get_specialize(), pack_sources=kc.get_pack_sources(),
                pack_budget_mb=kc.get_pack_budget_mb(), chain_quads=kc.get_chain_quads())


def _restore(kc):
    kc.specialize_wait()
    for n, v in _SAVED["options"].items():
        kc.set_option(n, v)
    kc.set_specialize(_SAVED["specialize"], 2)
    kc.set_pack_sources(_SAVED["pack_sources"])
    kc.set_pack_budget_mb(_SAVED["pack_budget_mb"])
    kc.set_chain_quads(_SAVED["chain_quads"])


def _snapshot(kc):
    d = {n: kc.stats_counter(n) for n in COUNTERS}
    d["q2"] = sum(kc.stats_counter(n) for n in Q2)
    d["pk"] = sum(kc.stats_counter(n) for n in PK)
    d.update(kc.specialize_stats())
    d["kernel_launches"] = kc.stats()["kernel_launches"]
    return d


@pytest.fixture(scope="module")
def kc(tmp_path_factory):
    import kanter_core_amd as kc
    kc.init(0)
    kc.specialize_wait()
    _SAVED.update(_switches(kc))
    kc.kernel_cache_set_dir(str(tmp_path_factory.mktemp("kernel_cache")))  # no stale code objects in, nothing into the home directory
    _BASE.update(_snapshot(kc))
    _BASE["t0"] = time.perf_counter()
    try:
        yield kc
    finally:
        _restore(kc)
        kc.kernel_cache_set_dir(None)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as orc
    return orc


@contextlib.contextmanager
def regime(kc, name, cache_policy):
    """The process-wide switches of a regime ("forced", "natural", "plain": everything off) and of a seed's cache policy."""
    failed0 = kc.specialize_stats()["compiles_failed"]
    try:
        kc.specialize_wait()
        kc.set_option("join", 0 if name == "plain" else 1)
        kc.set_option("replay", 0 if name == "plain" else 1)
        if name == "forced":
            kc.set_specialize(2)
            kc.set_pack_sources(2)
        elif name == "natural":
            kc.set_specialize(1, 2)
            kc.set_pack_sources(1)
        else:
            kc.set_specialize(0)
            kc.set_pack_sources(0)
        if name == "natural" or cache_policy == "budget0":
            kc.set_option("cache_budget_mb", 0)
        if cache_policy == "warm":
            kc.set_option("nt_force", 0x101)
        yield
        kc.specialize_wait()
        assert kc.specialize_stats()["compiles_failed"] == failed0, "a generated kernel did not compile"
    finally:
        _restore(kc)


REFUSED = "refused"


def _label(case):
    return hex(case.seed) if isinstance(case.seed, int) else case.seed


def run_once(kc, lg, case):
    """Re-plugs the sources and evaluates the requested node once more: -> ([(slot id, is_rgba, planes)] by slot id or REFUSED
    where the device raises, kernels compiled meanwhile); notes which counters the evaluation raised."""
    case.replug(lg)
    before = _snapshot(kc)
    try:
        got = [(int(s.slot_id), s.image.is_rgba(), s.image.planes())
               for s in sorted(lg.await_clean(case.root).node_slot_datas(case.root), key=lambda s: s.slot_id)]
    except kc.TexProError:
        got = REFUSED
    after = _snapshot(kc)
    for n in FLOORS:
        if after[n] > before[n] and isinstance(case.seed, int):  # (the sweeps' seeds: the reduced graphs do not count)
            SEEN[n].add(case.seed)
    if case.raw_planes >= 9 and after["wide_launches"] > before["wide_launches"] and after["kernel_launches"] - before["kernel_launches"] == 1:
        WIDE9.add(case.seed)
    return got, after["kernels_compiled"] - before["kernels_compiled"]


def lifecycle(kc, case, name, n_evaluations, want=None):
    """The case's live graph under the regime, evaluated n times; with `want` (the oracle's slot datas, REFUSED where it refuses
    the node) every evaluation is compared with it.  -> the last evaluation's result."""
    with regime(kc, name, case.cache_policy):
        lg = case.live_graph(kc)
        for i in range(n_evaluations):
            what = "seed %s, %s (%s), evaluation %d" % (_label(case), name, case.cache_policy, i)
            t0 = time.perf_counter()
            got, compiled = run_once(kc, lg, case)
            if name == "forced" and i == 0:
                COMPILE[0] += time.perf_counter() - t0
                COMPILE[1] += compiled
            if name == "natural":
                kc.specialize_wait()  # what was queued has landed before the next evaluation: the sequence is deterministic
            if want is None:
                continue
            if isinstance(want, str) or isinstance(got, str):
                assert isinstance(got, str) and isinstance(want, str), "%s: only one of device and oracle refuses the node" % what
                continue
            assert len(got) == len(want), what
            for (slot, rgba, planes), w in zip(got, want):
                assert slot == int(w.slot_id) and rgba == w.image.is_rgba, what
                assert_planes(planes, w.image.planes, what="%s slot %d" % (what, slot))
        return got


def _want(case):
    want = case.want()
    return REFUSED if want is None else want


@pytest.mark.parametrize("seed", range(sf.N_FORCED))
def test_forced_steady_state_matches_the_oracle(kc, orc, seed):
    case = sf.random_case(orc, sf.SEED_FORCED + seed)
    RAN.add(case.seed)
    lifecycle(kc, case, "forced", 4, _want(case))


@pytest.mark.parametrize("seed", range(sf.N_NATURAL))
def test_natural_steady_state_matches_the_oracle(kc, orc, seed):
    case = sf.random_case(orc, sf.SEED_NATURAL + seed)
    RAN.add(case.seed)
    lifecycle(kc, case, "natural", 6, _want(case))


@pytest.mark.parametrize("seed", range(sf.N_POW))
def test_pow_steady_state_equals_the_plain_path(kc, orc, seed):
    """Pow among the ops, device against device: the forced regime's fourth evaluation against one evaluation with kernels
    compiled for programs, packed sources, joins and replay all off."""
    case = sf.random_case(orc, sf.SEED_POW + seed, pow_ops=True)
    RAN.add(case.seed)
    steady, plain = lifecycle(kc, case, "forced", 4), lifecycle(kc, case, "plain", 1)
    what = "seed %#x (%s)" % (case.seed, case.cache_policy)
    if isinstance(steady, str) or isinstance(plain, str):
        assert isinstance(steady, str) and isinstance(plain, str), "%s: only one of the two paths refuses the node" % what
        return
    assert [s[:2] for s in steady] == [s[:2] for s in plain], what
    for (slot, _, a), (_, _, b) in zip(steady, plain):
        assert_planes(a, b, what="%s, slot %d, steady state against the plain path" % (what, slot))


@pytest.mark.parametrize("seed,name,n", [(sf.SEED_NATURAL + 14, "natural", 6)])
def test_seeds_that_found_defects(kc, orc, seed, name, n):
    """SEED_NATURAL + 14: a Mix of a chain that holds a join with a smaller image.  plane_mix kept the resampled operand in the
    joined chain's program (join_ok refused the other order only), so the program went to a fused resize + chain kernel: its step
    interpreter does not know CH_SAVE_LOAD and the generator of the compiled up-sampling kernel refuses it -- a compile failure and
    every pixel of the result wrong (1568 of 1568), from the first evaluation on in every mode but kc_set_specialize(0).  A chain
    that holds a join now runs before it meets a resampled operand (csrc/runtime.cpp, chain_full_with), and chain_resize_launch
    takes no program with that code.  Reduced: test_a_resampled_operand_behind_a_join."""
    case = sf.random_case(orc, seed)
    lifecycle(kc, case, name, n, _want(case))


REDUCED = [((16, 4), (64, 16), "Triangle"), ((16, 4), (64, 16), "Nearest"), ((24, 16), (64, 16), "Triangle"), ((1, 1), (128, 3), "Triangle"),
           ((5, 3), (17, 29), "CatmullRom")]


@pytest.mark.parametrize("small,big,filt", REDUCED, ids=["%dx%d-%dx%d-%s" % (c[0] + c[1] + (c[2],)) for c in REDUCED])
@pytest.mark.parametrize("name,n", [("forced", 4), ("natural", 6)])
def test_a_resampled_operand_behind_a_join(kc, orc, small, big, filt, name, n):
    """The defect of test_seeds_that_found_defects reduced: ((a + b) - (a * b)) + s with s smaller than a and b -- integer ratios (the fused
    up-sampling kernel), other ratios (the fused resize kernel), a 1 x 1 image and a filter neither fused kernel takes."""
    case = sf.joined_then_resampled(orc, small, big, filt)
    lifecycle(kc, case, name, n, _want(case))


def test_the_fuzz_reaches_every_steady_state_form(kc):
    """Every form's counter rose during the module, for at least 8 different seeds each, and some evaluation was ONE launch of a
    wide program over 9 or more distinct source planes; no generated kernel failed to compile."""
    if len(RAN) < sf.N_FORCED + sf.N_NATURAL + sf.N_POW:
        pytest.skip("only meaningful after the other tests of this module")
    now = _snapshot(kc)
    rise = {n: now[n] - _BASE[n] for n in FLOORS + ["kernels_compiled", "compiles_failed"]}
    print("seeds / rise: " + ", ".join("%s %d / %d" % (n, len(SEEN[n]), rise[n]) for n in FLOORS))
    print("one-launch programs of 9 or more planes: seeds %s" % sorted(hex(s) for s in WIDE9))
    print("kernels compiled %d; first forced evaluations: %.1f s for %d kernels; module %.0f s" % (
        rise["kernels_compiled"], COMPILE[0], COMPILE[1], time.perf_counter() - _BASE["t0"]))
    assert rise["compiles_failed"] == 0
    short = {n: (len(SEEN[n]), rise[n]) for n in FLOORS if rise[n] < 1 or len(SEEN[n]) < 8}
    assert not short, "forms reached by fewer than 8 seeds: %s" % short
    assert WIDE9, "no one-launch program of more than 8 input planes"


def test_every_switch_is_back_at_its_default(kc):
    assert _switches(kc) == _SAVED
    if not any("KC_" + n.upper() in os.environ for n in OPTIONS + ("specialize", "pack_sources", "chain_quads")):
        assert _SAVED == dict(options={"join": 1, "replay": 1, "cache_budget_mb": 208, "nt_force": -1}, specialize=1, pack_sources=1,
                              pack_budget_mb=_SAVED["pack_budget_mb"], chain_quads=0)
