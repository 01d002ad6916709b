"""What a change invalidates (csrc/evo_amd.hip: the validity section; DESIGN.md "What a change invalidates"): a fixed
script of public calls, the validity state after every step (Engine.debug_validity) against a table written out below,
the launches per kernel class at its end, and the public outputs of three steps against contexts that ran only the
steps needed to reach them.

The tables were recorded ONCE on the commit before the change events existed (only evoamd_debug_validity and its binding
applied to it): they say what the loose flags did, not what the events do.  A row is (step, the call raised, the bits of
out[0], gen, kn_gen, theta_gen, pending_skip, census_skip, kn_refill, pred_N)."""
import numpy as np
import pytest

import _estep_problems as ep
from test_gpu_context import ACC_ATOL, ACC_RTOL, BSC_LARGE, CMAX, ES_SMALL, LEARN, _problem, _set_params

pytestmark = pytest.mark.gpu

# the geometry a script ends on ("configure to the other geometry"); EBSC gets its permanent all-zero state there
OTHER = {"es3c": ("bsc", 64, 12, 8, 4, 1, CMAX), "bsc": ES_SMALL}
GEOM = {"es3c": ES_SMALL, "bsc": BSC_LARGE}
OUTPUT_STEPS = ("08 stats", "12 vary_kn", "18 stats")


def _script(p):
    """[(step name, f(eng, out))]: the script of the module docstring for the problem p."""
    model, n, D, H, S = p["geom"][:5]
    rng = np.random.RandomState(7)
    packed = np.packbits(p["ss"], axis=-1)
    keep = rng.random_sample((n, D)) < 0.5
    x_infr = rng.random_sample((n, D)) < 0.8
    cand = ep.make_kn(rng, n, CMAX, H, kmax=4)
    counts = np.full(n, CMAX, dtype=np.int32)
    cand_lpj = rng.normal(size=(n, CMAX))

    def outputs(eng, out, name, acc=None, F=None):
        views = {} if acc is None else {k: np.array(v) for k, v in dict(eng.acc_views(acc)).items()}
        out[name] = (eng.download_states(), eng.download_lpj(), views["Fs"] if F is None else F, views)

    def stats(name):
        return lambda eng, out: outputs(eng, out, name, acc=eng.stats())

    def vary(name):
        return lambda eng, out: outputs(eng, out, name, F=eng.vary_kn(S))

    def estep(fused, seed):
        def f(eng, out):
            eng.set_option("fused_estep", fused)
            eng.estep(2, 2, seed, True, S)
            eng.set_option("fused_estep", 0)
        return f

    steps = [
        ("01 configure", lambda eng, out: eng.configure(*p["geom"])),
        ("02 upload_data", lambda eng, out: eng.upload_data(p["Y"])),
        ("03 upload_states", lambda eng, out: eng.upload_states(p["ss"])),
        ("04 set_params", lambda eng, out: _set_params(eng, p)),
        ("05 lpj_resident", lambda eng, out: eng.lpj_resident()),
        ("06 evolve_randflip", lambda eng, out: eng.evolve_randflip(2, 2, 11)),
        ("07 vary_kn", lambda eng, out: eng.vary_kn(S)),
        ("08 stats", stats("08 stats")),
        ("09 mstep_device", lambda eng, out: eng.mstep_device(LEARN[model])),
        ("10 lpj_resident", lambda eng, out: eng.lpj_resident()),
        ("11 evolve_states", lambda eng, out: eng.evolve_states("randflip", 1, 2, 2, 13)),
        ("12 vary_kn", vary("12 vary_kn")),
        ("13 mstep_device lazy", lambda eng, out: eng.mstep_device(LEARN[model], theta_to_host=False)),
        ("14 restore_theta_backup", lambda eng, out: eng.restore_theta_backup()),
        ("15 set_params", lambda eng, out: _set_params(eng, p)),
        ("16 estep fused_estep=2", estep(2, 17)),
        ("17 estep fused_estep=0", estep(0, 19)),
        ("18 stats", stats("18 stats")),
        ("19 reconstruct", lambda eng, out: eng.reconstruct()),
        ("20 reconstruct_resident", lambda eng, out: eng.reconstruct_resident(keep)),
        ("21 posterior_codes", lambda eng, out: eng.posterior_codes(max_active=4)),
        ("22 upload_states_packed rows", lambda eng, out: eng.upload_states_packed(packed[8:24], 8)),
        ("23 init_states", lambda eng, out: eng.init_states(0.3, 17)),
        ("24 init_states max_rounds=1", lambda eng, out: eng.init_states(1.0 / H, 17, max_rounds=1)),
        ("25a refill first half", lambda eng, out: eng.upload_states_packed(packed[:32], 0)),
        ("25b refill second half", lambda eng, out: eng.upload_states_packed(packed[32:], 32)),
        ("26 set_candidates", lambda eng, out: eng.set_candidates(cand, counts, cand_lpj)),
        ("27 lpj_candidates", lambda eng, out: eng.lpj_candidates(cand, counts)),
        ("28a state_digest=0", lambda eng, out: eng.set_option("state_digest", 0)),
        ("28b state_digest=1", lambda eng, out: eng.set_option("state_digest", 1)),
    ]
    if model == "bsc":
        steps += [
            ("29a upload_masks", lambda eng, out: eng.upload_masks(x_infr)),
            ("29b set_reliable_fraction", lambda eng, out: eng.set_reliable_fraction(x_infr.sum() / float(n))),
            ("29c set_params", lambda eng, out: _set_params(eng, p)),
            ("29d lpj_resident", lambda eng, out: eng.lpj_resident()),
            ("29e upload_yrec", lambda eng, out: eng.upload_yrec(p["Y"])),
            ("29f stats", lambda eng, out: eng.stats()),
            ("29g upload_masks(None)", lambda eng, out: eng.upload_masks(None)),
        ]
    steps.append(("30 configure other", lambda eng, out: eng.configure(*OTHER[model])))
    return steps


def _row(name, raised, v):
    from evo_amd import _lib
    bits = sum(1 << i for i, k in enumerate(_lib.VALIDITY_BITS) if v[k])
    return (name, raised, bits) + tuple(v[k] for k in _lib.VALIDITY_WORDS)


def walk(model, only=None):
    """Run the script (the steps whose number is in ``only``, else all) on a context of its own.  Returns (rows, launches
    per kernel class in front of the last configure, {step: (K^n, lpj, F, accumulator views)})."""
    from evo_amd import _lib
    from evo_amd.engine import Engine, EvoAmdError
    p = _problem(GEOM[model], 21)
    eng = Engine()
    rows, out, counts = [], {}, None
    try:
        eng.timing(True)
        for name, f in _script(p):
            if only is not None and int(name[:2]) not in only:
                continue
            if name.startswith("30"):
                counts = {k: eng.kernel_time_ms(k)[1] for k in _lib.KERNEL_IDS}
            raised = False
            try:
                f(eng, out)
            except EvoAmdError:
                raised = True
            rows.append(_row(name, raised, eng.debug_validity()))
    finally:
        eng.close()
    return rows, counts, out


# ---- recorded on the parent commit (module docstring) ---------------------------------------------------------------
TABLE = {
    "es3c": [
        ("01 configure", False, 0x0001c000, 1, 2, 0, 0, 0, 0, 0),
        ("02 upload_data", False, 0x0001c001, 2, 2, 0, 0, 0, 0, 0),
        ("03 upload_states", False, 0x0001c001, 3, 3, 0, 0, 0, 0, 0),
        ("04 set_params", False, 0x0001c00b, 4, 3, 1, 0, 0, 0, 0),
        ("05 lpj_resident", False, 0x4001c00b, 4, 3, 1, 0, 0, 0, 0),
        ("06 evolve_randflip", False, 0x4003c00f, 4, 3, 1, 0, 0, 0, 0),
        ("07 vary_kn", False, 0x001fc01f, 5, 4, 1, 0, 0, 0, 0),
        ("08 stats", False, 0xc006603f, 5, 4, 1, 0, 0, 0, 0),
        ("09 mstep_device", False, 0xe042600f, 6, 4, 2, 2, 4, 0, 0),
        ("10 lpj_resident", False, 0xc042600f, 6, 4, 2, 2, 4, 0, 0),
        ("11 evolve_states", False, 0xc040600f, 6, 4, 2, 0, 4, 0, 0),
        ("12 vary_kn", False, 0x005c601f, 7, 5, 2, 0, 0, 0, 0),
        ("13 mstep_device lazy", False, 0xe080600f, 8, 5, 3, 2, 4, 0, 0),
        ("14 restore_theta_backup", False, 0xc0806007, 9, 5, 3, 2, 4, 0, 0),
        ("15 set_params", False, 0xc080600f, 10, 5, 4, 2, 4, 0, 0),
        ("16 estep fused_estep=2", False, 0x4682601b, 13, 6, 4, 2, 0, 0, 0),
        ("17 estep fused_estep=0", False, 0x049e601f, 16, 7, 4, 0, 0, 0, 0),
        ("18 stats", False, 0xc086603f, 16, 7, 4, 0, 0, 0, 0),
        ("19 reconstruct", False, 0xc086607f, 16, 7, 4, 0, 0, 0, 0),
        ("20 reconstruct_resident", False, 0xc08678ff, 16, 7, 4, 0, 0, 0, 0),
        ("21 posterior_codes", False, 0xc08678ff, 16, 7, 4, 0, 0, 0, 0),
        ("22 upload_states_packed rows", False, 0x008658ff, 17, 8, 4, 0, 0, 0, 0),
        ("23 init_states", False, 0x008658ff, 18, 9, 4, 0, 0, 0, 0),
        ("24 init_states max_rounds=1", True, 0x018658ff, 19, 10, 4, 0, 0, 0, 0),
        ("25a refill first half", False, 0x018658ff, 20, 11, 4, 0, 0, 32, 0),
        ("25b refill second half", False, 0x008658ff, 21, 12, 4, 0, 0, 64, 0),
        ("26 set_candidates", False, 0x008458ff, 21, 12, 4, 0, 0, 64, 0),
        ("27 lpj_candidates", False, 0x008058ff, 21, 12, 4, 0, 0, 64, 0),
        ("28a state_digest=0", False, 0x008058ff, 22, 12, 4, 0, 0, 64, 0),
        ("28b state_digest=1", False, 0x008058ff, 23, 12, 4, 0, 0, 64, 0),
        ("30 configure other", False, 0x00005008, 24, 13, 4, 0, 0, 64, 0),
    ],
    "bsc": [
        ("01 configure", False, 0x0001c000, 1, 2, 0, 0, 0, 0, 0),
        ("02 upload_data", False, 0x0001c001, 2, 2, 0, 0, 0, 0, 0),
        ("03 upload_states", False, 0x0001c001, 3, 3, 0, 0, 0, 0, 0),
        ("04 set_params", False, 0x0001c00b, 4, 3, 0, 0, 0, 0, 0),
        ("05 lpj_resident", False, 0x0001c00b, 4, 3, 0, 0, 0, 0, 0),
        ("06 evolve_randflip", False, 0x0003c00f, 4, 3, 0, 0, 0, 0, 0),
        ("07 vary_kn", False, 0x0013c01f, 5, 4, 0, 0, 0, 0, 0),
        ("08 stats", False, 0x8023c03f, 5, 4, 0, 0, 0, 0, 0),
        ("09 mstep_device", False, 0xa043c00f, 6, 4, 0, 0, 0, 0, 0),
        ("10 lpj_resident", False, 0x8043c00f, 6, 4, 0, 0, 0, 0, 0),
        ("11 evolve_states", False, 0x8041c00f, 6, 4, 0, 0, 0, 0, 0),
        ("12 vary_kn", False, 0x0051c01f, 7, 5, 0, 0, 0, 0, 0),
        ("13 mstep_device lazy", False, 0xa081c00f, 8, 5, 0, 0, 0, 0, 0),
        ("14 restore_theta_backup", False, 0x8081c007, 9, 5, 0, 0, 0, 0, 0),
        ("15 set_params", False, 0x8081c00f, 10, 5, 0, 0, 0, 0, 0),
        ("16 estep fused_estep=2", False, 0x0093c01f, 13, 6, 0, 0, 0, 0, 0),
        ("17 estep fused_estep=0", False, 0x0093c01f, 16, 7, 0, 0, 0, 0, 0),
        ("18 stats", False, 0x80a3c03f, 16, 7, 0, 0, 0, 0, 0),
        ("19 reconstruct", False, 0x80a3c07f, 16, 7, 0, 0, 0, 0, 0),
        ("20 reconstruct_resident", False, 0x80a3d8ff, 16, 7, 0, 0, 0, 0, 0),
        ("21 posterior_codes", False, 0x80a3d8ff, 16, 7, 0, 0, 0, 0, 0),
        ("22 upload_states_packed rows", False, 0x00a3d8ff, 17, 8, 0, 0, 0, 0, 0),
        ("23 init_states", False, 0x00a3d8ff, 18, 9, 0, 0, 0, 0, 0),
        ("24 init_states max_rounds=1", True, 0x01a3d8ff, 19, 10, 0, 0, 0, 0, 0),
        ("25a refill first half", False, 0x01a3d8ff, 20, 11, 0, 0, 0, 32, 0),
        ("25b refill second half", False, 0x00a3d8ff, 21, 12, 0, 0, 0, 64, 0),
        ("26 set_candidates", False, 0x00a1d8ff, 21, 12, 0, 0, 0, 64, 0),
        ("27 lpj_candidates", False, 0x00a1d8ff, 21, 12, 0, 0, 0, 64, 0),
        ("28a state_digest=0", False, 0x00a1d8ff, 22, 12, 0, 0, 0, 64, 0),
        ("28b state_digest=1", False, 0x00a1d8ff, 23, 12, 0, 0, 0, 64, 0),
        ("29a upload_masks", False, 0x00a1d877, 23, 12, 0, 0, 0, 64, 0),
        ("29b set_reliable_fraction", False, 0x00a1d877, 23, 12, 0, 0, 0, 64, 0),
        ("29c set_params", False, 0x00a1d81f, 24, 12, 0, 0, 0, 64, 0),
        ("29d lpj_resident", False, 0x00a1d80f, 24, 12, 0, 0, 0, 64, 0),
        ("29e upload_yrec", False, 0x00a1d90f, 24, 12, 0, 0, 0, 64, 0),
        ("29f stats", False, 0x8081d92f, 24, 12, 0, 0, 0, 64, 0),
        ("29g upload_masks(None)", False, 0x8081d82f, 24, 12, 0, 0, 0, 64, 0),
        ("30 configure other", False, 0x0001d008, 25, 13, 0, 0, 0, 64, 0),
    ],
}
LAUNCHES = {
    "es3c": {"allreduce": 0,
     "estep_fused": 1,
     "evolve": 4,
     "gemm_f64": 13,
     "init_states": 2,
     "lpj_candidates": 5,
     "lpj_k3_4": 5,
     "lpj_k5_8": 1,
     "lpj_k9plus": 5,
     "lpj_overflow": 10,
     "lpj_pass": 5,
     "lpj_resident": 4,
     "misc": 13,
     "mstep_device": 4,
     "patches": 0,
     "row_lse": 0,
     "stats": 4,
     "stats_k3_4": 4,
     "stats_k5_8": 2,
     "stats_k9plus": 4,
     "stats_overflow": 8,
     "stats_pass": 4,
     "vary_kn": 3},
    "bsc": {"allreduce": 0,
     "estep_fused": 0,
     "evolve": 5,
     "gemm_f64": 16,
     "init_states": 2,
     "lpj_candidates": 6,
     "lpj_k3_4": 0,
     "lpj_k5_8": 0,
     "lpj_k9plus": 0,
     "lpj_overflow": 0,
     "lpj_pass": 6,
     "lpj_resident": 6,
     "misc": 11,
     "mstep_device": 4,
     "patches": 0,
     "row_lse": 1,
     "stats": 5,
     "stats_k3_4": 0,
     "stats_k5_8": 0,
     "stats_k9plus": 0,
     "stats_overflow": 0,
     "stats_pass": 5,
     "vary_kn": 4},
}


def _describe(got, want):
    from evo_amd import _lib
    diff = [k for i, k in enumerate(_lib.VALIDITY_BITS) if (got[2] ^ want[2]) >> i & 1]
    diff += [k for k, a, b in zip(_lib.VALIDITY_WORDS, got[3:], want[3:]) if a != b]
    return "%s: differs in %s (got %r, recorded %r)" % (got[0], ", ".join(diff) or "raised", got, want)


@pytest.fixture(scope="module", params=("es3c", "bsc"))
def walked(request):
    return (request.param,) + walk(request.param)


def test_every_step_leaves_the_recorded_validity_state(walked):
    model, rows, _, _ = walked
    assert [r[0] for r in rows] == [r[0] for r in TABLE[model]]
    wrong = [_describe(g, w) for g, w in zip(rows, TABLE[model]) if g != w]
    assert not wrong, "\n".join(wrong)


def test_no_launch_was_added_dropped_or_rerouted(walked):
    model, _, counts, _ = walked
    assert counts == LAUNCHES[model]


def test_outputs_equal_contexts_that_ran_only_the_steps_needed(walked):
    """K^n exactly; lpj, F and the accumulator views within the bound two device runs of the same statistics kernels are
    held to (test_gpu_context.py).  Step 8 needs steps 1-7; step 12 steps 1-7 and 9-11 (the statistics of step 8 are
    formed again by the Theta update); step 18 those and 15-17 (the lazy update and its restore are undone by step 15)."""
    model, _, _, out = walked
    short = walk(model, only=set(range(1, 9)))[2]
    long = walk(model, only=set(range(1, 8)) | set(range(9, 13)) | set(range(15, 19)))[2]
    for name, want in ((OUTPUT_STEPS[0], short), (OUTPUT_STEPS[1], long), (OUTPUT_STEPS[2], long)):
        got_kn, got_lpj, got_F, got_views = out[name]
        want_kn, want_lpj, want_F, want_views = want[name]
        assert np.array_equal(got_kn, want_kn), name
        np.testing.assert_allclose(got_lpj, want_lpj, rtol=ACC_RTOL, atol=ACC_ATOL, err_msg=name)
        np.testing.assert_allclose(got_F, want_F, rtol=ACC_RTOL, atol=ACC_ATOL, err_msg=name)
        assert sorted(got_views) == sorted(want_views)
        for k in want_views:
            np.testing.assert_allclose(got_views[k], want_views[k], rtol=ACC_RTOL, atol=ACC_ATOL, err_msg=name + " " + k)
