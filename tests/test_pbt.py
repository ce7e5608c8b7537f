"""Population-based training on the device (csrc/acas2d_pbt.hip): acas2d_member_episodes_f32 scores the members of a
population from a collection's [T][E] buffers, acas2d_population_exploit_f32 ranks them, copies better members into the
worst and perturbs the copied hyper row -- two launches, no host decision.

The exploit contract is bitwise and its rules are normative (include/acas2d.h); tests/pbt_ref.py restates them in NumPy
on oracle.philox4x32, and the CPU tests pin that referee on hand-computed cases first.  The episode sums are held to exact
integers and to the worst-case bound of a double summation in any order.  PBTTrainer is held to PopulationTrainer (no
exchange: the same bits) and to the referee applied to a snapshot (with exchange)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import pbt_ref as R

torch = pytest.importorskip("torch")
DEV = "cuda:0"
WIDTHS = (8, 11, 14, 17, 29, 53, 101, 197)
INT32_MIN = np.iinfo(np.int32).min
F32 = np.float32


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g.native.lib()
    return g


def ubits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- CPU: the referee on hand-computed cases -----------------------------------------------------------------------------
def test_referee_ranks_are_a_total_order_with_nan_last_and_ties_by_index():
    """By the rule of include/acas2d.h: key = -inf for a NaN score, rank = members with a greater key + members with an
    equal key and a smaller index.  [3, NaN, 3, -inf] has the keys [3, -inf, 3, -inf]: the two 3s take ranks 0 and 1 by
    index, and the NaN of member 1 ties with the -inf of member 3 and wins by index, 2 before 3.  (A NaN is never ranked
    BELOW a -inf of a smaller or greater index: it is one, by the key.)"""
    assert list(R.ranks([3, np.nan, 3, -np.inf])) == [0, 2, 1, 3]
    assert list(R.ranks([3, -np.inf, 3, np.nan])) == [0, 2, 1, 3]
    assert list(R.ranks([np.nan, np.nan, np.nan])) == [0, 1, 2]
    assert list(R.ranks([0.0, -0.0, 1.0, -0.0])) == [1, 2, 0, 3]            # +0 == -0: the index decides
    assert list(R.ranks([-np.inf, np.nan, np.inf])) == [1, 2, 0]            # NaN counts as -inf and loses the tie to 0
    rng = np.random.default_rng(3)
    for K in (1, 2, 7, 64):
        s = rng.integers(-2, 3, K).astype(F32)
        assert sorted(R.ranks(s)) == list(range(K))


def test_referee_target_rank_is_uniform_over_the_donors():
    """rho = (w.x * R) >> 32 over 10 000 counters, R = 8: Pearson's chi-square with 7 degrees of freedom stays below its
    1 - 1e-4 quantile, 29.88 (Abramowitz & Stegun 26.4: P(chi2_7 > 29.88) = 1e-4)."""
    n, Rr = 10000, 8
    counts = np.zeros(Rr, np.int64)
    for k in range(n):
        rho = R.target_rank(R.words(k % 1000, k // 1000, 0x123456789abcdef)[0], Rr)
        assert 0 <= rho < Rr
        counts[rho] += 1
    chi2 = float(((counts - n / Rr) ** 2 / (n / Rr)).sum())
    print("counts", counts, "chi2", chi2)
    assert chi2 < 29.88
    assert R.target_rank(0xffffffff, 5) == 4 and R.target_rank(0, 5) == 0 and R.target_rank(0x80000000, 1) == 0


def test_referee_words_are_the_pinned_generator_on_the_documented_counter():
    from oracle import oracle as O
    w = R.words(5, 2, (7 << 32) | 9)
    assert list(w) == list(O.philox4x32([5, 2, 0, 0x70627431], [9, 7])) and O.RESET_PHILOX_ROUNDS == 7
    assert list(w) != list(R.words(5, 3, (7 << 32) | 9)) and list(w) != list(R.words(5, 2, (7 << 32) | 10))


def test_referee_perturbs_into_bounds_and_copies_unmasked_slots_bitwise():
    rng = np.random.default_rng(11)
    K, Rr = 16, 8
    hyper = rng.uniform(1e-4, 1.0, (K, 8)).astype(F32)
    hyper[3, 5] = np.float32(np.nan)                      # an unmasked NaN payload must survive as it is
    hyper.view(np.uint32)[3, 5] = 0x7fc12345
    score = rng.permutation(K).astype(F32)
    lo, hi = np.full(8, 0.2, F32), np.full(8, 0.5, F32)
    mask = 0b00010101
    copies = 0
    for gen in range(20):
        donor, out = R.exploit(score, hyper, Rr, gen, 99, mask, 0.8, 1.2, lo, hi)
        rank = R.ranks(score)
        for k in range(K):
            if rank[k] < K - Rr:
                assert donor[k] == k and np.array_equal(out[k].view(np.uint32), hyper[k].view(np.uint32))
                continue
            d = donor[k]
            assert d != k and rank[d] < Rr              # distinct scores: every recipient copies one of the R best
            copies += 1
            for s in range(8):
                if (mask >> s) & 1:
                    assert lo[s] <= out[k, s] <= hi[s]
                    both = {float(np.clip(F32(hyper[d, s]) * F32(f), lo[s], hi[s])) for f in (0.8, 1.2)}
                    assert float(out[k, s]) in both
                else:
                    assert out[k].view(np.uint32)[s] == hyper[d].view(np.uint32)[s]
    assert copies == 20 * Rr
    # one float32 multiplication, then the clamp: 0.25 x 1.2 in float32, and a product past hi lands on hi
    assert R.perturbed(0.25, 1, 0.8, 1.2, 0.0, 1.0) == F32(0.25) * F32(1.2)
    assert R.perturbed(0.45, 1, 0.8, 1.2, 0.2, 0.5) == F32(0.5) and R.perturbed(0.21, 0, 0.8, 1.2, 0.2, 0.5) == F32(0.2)


def test_referee_never_copies_from_a_member_that_is_not_strictly_better():
    hyper = np.arange(32, dtype=F32).reshape(4, 8)
    lo, hi = np.zeros(8, F32), np.full(8, 100, F32)
    for score in ([1, 1, 1, 1], [np.nan] * 4, [np.nan, -np.inf, np.nan, -np.inf]):
        donor, out = R.exploit(score, hyper, 2, 0, 1, 0xff, 0.8, 1.2, lo, hi)
        assert list(donor) == [0, 1, 2, 3] and np.array_equal(out, hyper)
    donor, _ = R.exploit([np.nan, 5, np.nan, np.nan], hyper, 1, 0, 1, 0xff, 0.8, 1.2, lo, hi)
    assert list(donor) == [0, 1, 2, 1]                    # the one recipient (rank 3) takes the one donor


def test_referee_episode_sums_by_hand():
    done = np.array([[1, 0, 0, 1], [0, 0, 1, 1]], bool)
    outcome = np.array([[2, 9, 9, 0], [9, 9, 3, 3]], np.uint8)
    ret = np.array([[1.5, np.nan, np.inf, -2.0], [np.nan, np.nan, 4.0, 0.25]], F32)
    steps = np.array([[11, INT32_MIN, INT32_MIN, 3], [INT32_MIN, INT32_MIN, 5, 2]], np.int32)
    one = R.episodes(done, outcome, ret, steps, 1)
    assert one["count"][0] == 4 and list(one["outcomes"][0]) == [1, 0, 1, 2] and one["steps"][0] == 17
    assert one["return_sum"][0] == 3.75 and one["abs_sum"][0] == 7.75


# ---- CPU: the C ABI without a device --------------------------------------------------------------------------------------
ROWS = ("actor_w1", "actor_b1", "actor_w2", "actor_b2", "actor_w3", "actor_b3", "critic_w1", "critic_b1", "critic_w2",
        "critic_b2", "critic_w3", "critic_b3", "log_std", "adam_m", "adam_v")
EXPLOIT_POINTERS = ROWS + ("adam_step", "hyper", "score", "donor")
EPISODE_POINTERS = ("done", "outcome", "ep_return", "ep_steps", "ep_count", "ep_outcomes", "ep_steps_sum", "ep_return_sum",
                    "score")


def _valid_exploit(native, **over):
    """A struct every check accepts (made-up addresses: nothing may be launched with it), then `over`."""
    f = {n: 0x1000 * (i + 1) for i, n in enumerate(EXPLOIT_POINTERS)}
    f.update(n_members=8, obs_dim=8, n_replace=2, generation=0, seed=1, perturb_mask=0b00010101, factor_lo=0.8,
             factor_hi=1.2, lo=(C.c_float * 8)(*[0.0] * 8), hi=(C.c_float * 8)(*[1.0] * 8), _pad=0)
    f.update(over)
    return native.CPopulationExploit(**f)


def _valid_episodes(native, **over):
    f = {n: 0x1000 * (i + 1) for i, n in enumerate(EPISODE_POINTERS)}
    f.update(n_envs=192, n_steps=8, n_members=3)
    f.update(over)
    return native.CMemberEpisodes(**f)


def test_struct_sizes_match_their_ctypes_twins():
    from gym_acas2d_amd import native
    L = native.lib()
    assert L.acas2d_member_episodes_size() == C.sizeof(native.CMemberEpisodes)
    assert L.acas2d_population_exploit_size() == C.sizeof(native.CPopulationExploit)
    for name in ("acas2d_member_episodes_f32", "acas2d_member_episodes_size", "acas2d_population_exploit_f32",
                 "acas2d_population_exploit_size"):
        assert name in native.EXPORTS


def test_exploit_rejections_without_a_device():
    from gym_acas2d_amd import native
    L = native.lib()
    bad = lambda slot, l, h: dict(lo=(C.c_float * 8)(*[l if s == slot else 0.0 for s in range(8)]),  # noqa: E731
                                  hi=(C.c_float * 8)(*[h if s == slot else 1.0 for s in range(8)]))
    cases = [("NULL struct", None)] + [("NULL " + n, {n: None}) for n in EXPLOIT_POINTERS]
    cases += [("obs_dim %d" % d, dict(obs_dim=d)) for d in (0, 7, 9, 30, 198, -8)]
    cases += [("n_members %d" % k, dict(n_members=k, n_replace=0)) for k in (0, -1, 1025, 65535)]
    cases += [("n_replace -1", dict(n_replace=-1)), ("2R > K", dict(n_replace=5)), ("2R > K, K odd", dict(n_members=7, n_replace=4)),
              ("R huge", dict(n_replace=2 ** 31 - 1))]
    for name in ("factor_lo", "factor_hi"):
        cases += [("%s = %r" % (name, v), {name: v}) for v in (0.0, -0.8, float("inf"), float("nan"))]
    cases += [("lo > hi on a masked slot", bad(2, 0.6, 0.5)), ("NaN bound on a masked slot", bad(4, float("nan"), 0.5))]
    for out in ("donor", "score"):
        for name in EXPLOIT_POINTERS:
            if name != out:
                cases.append(("%s == %s" % (out, name), {out: _valid_exploit(native).__getattribute__(name)}))
    for what, over in cases:
        rc = (L.acas2d_population_exploit_f32(None, None) if over is None else
              L.acas2d_population_exploit_f32(C.byref(_valid_exploit(native, **over)), None))
        assert rc == -22, (what, rc)
        assert L.acas2d_last_error().startswith(b"acas2d_population_exploit") and len(L.acas2d_last_error()) > 30, what
    L.acas2d_population_exploit_f32(C.byref(_valid_exploit(native, n_replace=5)), None)
    assert b"n_replace" in L.acas2d_last_error()


def test_episodes_rejections_without_a_device():
    from gym_acas2d_amd import native
    L = native.lib()
    cases = [("NULL struct", None)] + [("NULL " + n, {n: None}) for n in EPISODE_POINTERS]
    cases += [("n_steps 0", dict(n_steps=0)), ("n_envs 0", dict(n_envs=0, n_members=1)), ("n_members 0", dict(n_members=0)),
              ("n_members 65536", dict(n_members=65536, n_envs=65536 * 64)), ("K = 3, EM = 65", dict(n_envs=195)),
              ("K = 2, odd split", dict(n_members=2, n_envs=193)), ("n_envs 2^31", dict(n_members=1, n_envs=2 ** 31))]
    for what, over in cases:
        rc = (L.acas2d_member_episodes_f32(None, None) if over is None else
              L.acas2d_member_episodes_f32(C.byref(_valid_episodes(native, **over)), None))
        assert rc == -22, (what, rc)
        assert L.acas2d_last_error().startswith(b"acas2d_member_episodes") and len(L.acas2d_last_error()) > 30, what


def test_pbt_config_says_which_rule_it_holds():
    from gym_acas2d_amd.ppo import PBT_BOUNDS, PBTConfig
    c = PBTConfig(ready_every=4)
    assert (c.fraction, tuple(c.factors), tuple(c.perturb), c.seed) == (0.25, (0.8, 1.2),
                                                                        ("learning_rate", "clip_range", "ent_coef"), 0)
    assert c.bounds == {"learning_rate": (1e-6, 1e-2), "clip_range": (0.02, 0.5), "ent_coef": (0.0, 0.1)} == PBT_BOUNDS
    assert [c.n_replace(K) for K in (1, 3, 4, 7, 8, 16)] == [0, 0, 1, 1, 2, 4]
    assert PBTConfig(1, fraction=0.5).n_replace(5) == 2 and PBTConfig(1, fraction=0).n_replace(8) == 0
    with pytest.raises(ValueError, match="2 x n_replace <= K"):
        PBTConfig(1, fraction=0.75).n_replace(4)
    with pytest.raises(ValueError, match="2 x n_replace <= K"):
        PBTConfig(1, fraction=0.6).n_replace(5)
    for kw, match in ((dict(ready_every=0), "ready_every"), (dict(ready_every=1.5), "ready_every"),
                      (dict(ready_every=1, fraction=-0.1), "fraction"), (dict(ready_every=1, factors=(0.8, 0.0)), "factors"),
                      (dict(ready_every=1, factors=(0.8,)), "factors"), (dict(ready_every=1, perturb=("gamma",)), "hyper row"),
                      (dict(ready_every=1, perturb=("vf_coef",)), "bounds"),
                      (dict(ready_every=1, bounds={**PBT_BOUNDS, "clip_range": (0.5, 0.02)}), "bounds")):
        with pytest.raises(ValueError, match=match):
            PBTConfig(**kw)


@H.needs_hipcc
def test_pbt_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """The code-object metadata of csrc/acas2d_pbt.hip, read the way tests/test_gae_kernel.py reads its unit."""
    _, kernels = H.kernel_metadata(tmp_path, "acas2d_pbt.hip")
    assert len(kernels) == 2
    for k in kernels:
        assert "member_episodes_kernel" in k.name or "population_exploit_kernel" in k.name
        print(k.name, "vgpr", k.field("vgpr_count"), "sgpr", k.field("sgpr_count"))
        assert k.field("vgpr_spill_count") == 0 and k.field("sgpr_spill_count") == 0, k.name
        assert k.field("private_segment_fixed_size") == 0 and k.field("vgpr_count") <= 128, k.name


# ---- GPU: exploit against the referee, bit for bit -------------------------------------------------------------------------
def _row_lengths(native, D):
    net = [64 * D, 64, 64 * 64, 64, 64, 1]
    ws = int(native.lib().acas2d_ppo_workspace_floats(D))
    assert ws == 2 * sum(net) + 1 and ws % 2 == 1
    return net + net + [1, ws, ws]


class _Guarded:
    """K rows of `n` 4-byte words between two guards of random words; the front guard's length sets the alignment of the
    rows' base (4, 8, 12 or 0 bytes past a 16-byte boundary)."""

    def __init__(self, K, n, front, dev, values=None, dtype=torch.int32):
        self.K, self.n, self.front, self.back = K, n, front, 64
        total = front + K * n + self.back
        self.pristine = torch.randint(-2 ** 31, 2 ** 31, (total,), device=dev, dtype=torch.int64).to(torch.int32)
        if values is not None:
            self.body(self.pristine).copy_(torch.as_tensor(values).contiguous().view(torch.int32).reshape(K, n))
        self.work = self.pristine.clone()
        self.dtype = dtype

    def body(self, flat):
        return flat[self.front:self.front + self.K * self.n].view(self.K, self.n)

    @property
    def ptr(self):
        return self.work.data_ptr() + 4 * self.front

    def restore(self):
        self.work.copy_(self.pristine)

    def guards_intact(self):
        end = self.front + self.K * self.n
        return torch.equal(self.work[:self.front], self.pristine[:self.front]) and \
            torch.equal(self.work[end:], self.pristine[end:])


def _scores(K, rng):
    distinct = rng.permutation(K).astype(F32) - F32(K // 3)
    out = {"distinct": distinct, "all_equal": np.full(K, 1.5, F32), "ties_across_the_cut": np.floor(distinct / 3).astype(F32),
           "all_nan": np.full(K, np.nan, F32)}
    one_nan = distinct.copy()
    one_nan[K // 2] = np.nan
    infs = distinct.copy()
    infs[0], infs[K - 1] = np.inf, -np.inf
    zeros = np.where(rng.random(K) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    zeros[rng.random(K) < 0.2] = 1.0
    zeros[rng.random(K) < 0.2] = -1.0
    out.update(one_nan=one_nan, infs=infs, signed_zeros=zeros)
    return out


def _exploit_case(native, K, D, dev, seed):
    rng = np.random.default_rng(seed)
    rows = [_Guarded(K, n, 61 + i % 4, dev) for i, n in enumerate(_row_lengths(native, D))]
    step = _Guarded(K, 1, 63, dev, values=torch.as_tensor(rng.integers(0, 10 ** 6, K).astype(np.int32)))
    hyper0 = rng.uniform(1e-4, 1.0, (K, 8)).astype(F32)
    hyper = _Guarded(K, 8, 61, dev, values=torch.as_tensor(hyper0))
    donor = _Guarded(K, 1, 62, dev)
    return rows, step, hyper, hyper0, donor


def _launch_exploit(native, rows, step, hyper, score_d, donor, K, D, Rr, gen, seed, mask, lo, hi, flo=0.8, fhi=1.2):
    x = native.CPopulationExploit(*[r.ptr for r in rows], step.ptr, hyper.ptr, score_d.data_ptr(), donor.ptr, K, D, Rr, gen,
                                  seed, mask, flo, fhi, (C.c_float * 8)(*lo), (C.c_float * 8)(*hi), 0)
    native.check(native.lib().acas2d_population_exploit_f32(
        C.byref(x), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("D", (8, 197))
@pytest.mark.parametrize("K", (1, 2, 3, 5, 64, 65, 257))
def test_exploit_equals_the_referee_bitwise(g, K, D):
    """Every stack, adam_m, adam_v, adam_step, hyper and donor after the launch equal the referee's, word for word; the
    rows are random words (NaN patterns included), their bases 4, 8, 12 and 0 bytes past a 16-byte boundary, and the
    guards around every written buffer stay as they were.  n_replace in {0, 1, K // 2} x seven score vectors."""
    native, dev = g.native, torch.device(DEV)
    rows, step, hyper, hyper0, donor = _exploit_case(native, K, D, dev, seed=1000 * K + D)
    lo, hi = np.full(8, 0.05, F32), np.full(8, 0.6, F32)
    bufs = rows + [step, hyper, donor]
    case = 0
    for Rr in sorted({0, min(1, K // 2), K // 2}):
        for name, score in _scores(K, np.random.default_rng(K + 7 * Rr)).items():
            case += 1
            gen, seed, mask = case, (0x9e3779b9 << 32) | (K * 131 + case), (0b00010101, 0xff, 0x00)[case % 3]
            what = (K, D, Rr, name)
            for b in bufs:
                b.restore()
            _launch_exploit(native, rows, step, hyper, torch.as_tensor(score, device=dev), donor, K, D, Rr, gen, seed, mask,
                            lo, hi)
            d_ref, h_ref = R.exploit(score, hyper0, Rr, gen, seed, mask, 0.8, 1.2, lo, hi)
            rank = R.ranks(score)
            copied = d_ref != np.arange(K)
            assert not copied[rank < K - Rr].any(), what
            if name == "distinct" and Rr >= 1:
                assert copied.sum() == Rr, what              # every recipient has a strictly better donor
            if name in ("all_equal", "all_nan") or Rr == 0:
                assert not copied.any(), what
            assert np.array_equal(donor.body(donor.work).view(K).cpu().numpy(), d_ref), what
            assert np.array_equal(hyper.body(hyper.work).cpu().numpy().view(np.uint32), h_ref.view(np.uint32)), what
            sel = torch.as_tensor(d_ref.astype(np.int64), device=dev)
            for i, b in enumerate(rows + [step]):
                assert torch.equal(b.body(b.work), b.body(b.pristine)[sel]), what + (i,)
                # whoever did not copy is untouched in every bit (the same statement, spelled out)
                keep = torch.as_tensor(~copied, device=dev)
                assert torch.equal(b.body(b.work)[keep], b.body(b.pristine)[keep]), what + (i,)
            keep = ~copied
            assert np.array_equal(hyper.body(hyper.work).cpu().numpy().view(np.uint32)[keep], hyper0.view(np.uint32)[keep]), what
            for i, b in enumerate(bufs):
                assert b.guards_intact(), what + (i,)


@pytest.mark.gpu
def test_exploit_draws_depend_on_generation_and_seed(g):
    native, dev = g.native, torch.device(DEV)
    K, D, Rr = 65, 8, 32
    rows, step, hyper, hyper0, donor = _exploit_case(native, K, D, dev, seed=5)
    score = np.random.default_rng(2).permutation(K).astype(F32)
    lo, hi = np.zeros(8, F32), np.ones(8, F32)
    seen = {}
    for gen, seed in ((0, 1), (1, 1), (0, 2)):
        for b in rows + [step, hyper, donor]:
            b.restore()
        _launch_exploit(native, rows, step, hyper, torch.as_tensor(score, device=dev), donor, K, D, Rr, gen, seed, 0x15, lo, hi)
        seen[gen, seed] = donor.body(donor.work).view(K).cpu().numpy().copy()
        assert np.array_equal(seen[gen, seed], R.exploit(score, hyper0, Rr, gen, seed, 0x15, 0.8, 1.2, lo, hi)[0])
    assert not np.array_equal(seen[0, 1], seen[1, 1]) and not np.array_equal(seen[0, 1], seen[0, 2])


# ---- GPU: episodes against float64 NumPy ----------------------------------------------------------------------------------
EP_PATTERNS = ("none", "all", "one_env", "last_column", "random")


def _episode_inputs(T, E, K, pattern, seed):
    rng = np.random.default_rng(seed)
    EM = E // K
    done = np.zeros((T, E), bool)
    if pattern == "all":
        done[:] = True
    elif pattern == "one_env":
        done[:, E // 2] = True
    elif pattern == "last_column":
        done[:, EM - 1::EM] = True
    elif pattern == "random":
        done = rng.random((T, E)) < 0.3
    ret = (rng.normal(0, 1e3, (T, E))).astype(F32)        # magnitude 1e3, both signs
    steps = rng.integers(1, 500, (T, E)).astype(np.int32)
    outcome = rng.integers(0, 4, (T, E)).astype(np.uint8)
    poison = np.resize(np.array([np.nan, np.inf, -np.inf], F32), T * E).reshape(T, E)
    ret[~done] = poison[~done]                            # "written only where done": whatever lies elsewhere
    steps[~done] = INT32_MIN
    outcome[~done] = rng.integers(0, 256, (T, E)).astype(np.uint8)[~done]
    return done, outcome, ret, steps


def _check_episodes(g, T, E, K):
    dev = torch.device(DEV)
    d = lambda x: torch.as_tensor(x, device=dev)  # noqa: E731
    for pi, pattern in enumerate(EP_PATTERNS):
        done, outcome, ret, steps = _episode_inputs(T, E, K, pattern, seed=31 * T + E + pi)
        ref = R.episodes(done, outcome, ret, steps, K)
        args = (d(done), d(outcome), d(ret), d(steps), K)
        acc = g.member_episodes(*args)
        torch.cuda.synchronize()
        got = {n: t.cpu().numpy().copy() for n, t in acc.items()}
        what = (T, E, K, pattern)
        for n in ("count", "outcomes", "steps"):
            assert got[n].dtype == np.int64 and np.array_equal(got[n], ref[n]), what + (n,)
        bound = ref["count"] * 2.0 ** -53 * ref["abs_sum"]
        err = np.abs(got["return_sum"] - ref["return_sum"])
        print(what, "max error", err.max(), "bound", bound.max())
        assert got["return_sum"].dtype == np.float64 and (err <= bound).all(), what
        with np.errstate(invalid="ignore", divide="ignore"):
            want = (got["return_sum"] / got["count"].astype(np.float64)).astype(F32)
        real = ~np.isnan(want)
        assert got["score"].dtype == F32 and np.array_equal(np.isnan(got["score"]), ~real), what
        assert np.array_equal(got["score"][real].view(np.uint32), want[real].view(np.uint32)), what
        assert np.array_equal(np.isnan(got["score"]), ref["count"] == 0), what
        # two runs from zeroed accumulators agree in every bit
        again = g.member_episodes(*args)
        for n in acc:
            a, b = acc[n].cpu().numpy(), again[n].cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what + (n,)
        # a second call on the same accumulators doubles the integers exactly
        g.member_episodes(*args, acc=acc)
        for n in ("count", "outcomes", "steps"):
            assert np.array_equal(acc[n].cpu().numpy(), 2 * ref[n]), what + (n,)
        assert (np.abs(acc["return_sum"].cpu().numpy() - 2 * ref["return_sum"]) <= 2 * bound).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("EM", (64, 192))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("T", (1, 2, 17))
def test_member_episodes_equal_numpy(g, T, K, EM):
    _check_episodes(g, T, K * EM, K)


@pytest.mark.gpu
@pytest.mark.parametrize("E", (1, 63, 65, 1300))
def test_member_episodes_of_one_member_take_any_width(g, E):
    """K == 1: any n_envs; 1 300 columns run the four-chunk body (1 024), a partial one and the 64-column tail."""
    for T in (1, 2, 17):
        _check_episodes(g, T, E, 1)


@pytest.mark.gpu
def test_member_episodes_nan_return_stays_with_its_member(g):
    dev = torch.device(DEV)
    T, K, EM = 17, 3, 64
    done, outcome, ret, steps = _episode_inputs(T, K * EM, K, "random", seed=4)
    done[5, EM + 7] = True
    ret[5, EM + 7] = np.nan
    acc = g.member_episodes(*(torch.as_tensor(x, device=dev) for x in (done, outcome, ret, steps)), K)
    s, score = acc["return_sum"].cpu().numpy(), acc["score"].cpu().numpy()
    assert list(np.isnan(s)) == [False, True, False] and list(np.isnan(score)) == [False, True, False]
    ref = R.episodes(done, outcome, ret, steps, K)
    assert np.array_equal(acc["count"].cpu().numpy(), ref["count"])


# ---- GPU: the trainer ------------------------------------------------------------------------------------------------------
def _trainer(g, pbt, N=1, group=False, K=3, EM=64, T=2, B=64, gae=None, max_steps=None, epochs=2):
    cfgs = [g.PPOConfig(seed=13 + k, learning_rate=3e-4 * (1 + k), ent_coef=0.01 * k, n_steps=T, batch_size=B, n_epochs=epochs)
            for k in range(K)]
    conf = g.ACAS2DConfig(n_traffic=N, **({} if max_steps is None else {"max_steps": max_steps}))
    venv = g.ACAS2DVecEnv(K * EM, N, device=DEV, dtype=torch.float32, seed=13, config=conf)
    if pbt is None:
        return g.PopulationTrainer(venv, cfgs, gae=gae, group=group)
    return g.PBTTrainer(venv, cfgs, pbt, gae=gae, group=group)


def _state(t):
    fu = t._fused_update
    out = {n: p for n, p in t.policy_set.params.items()}
    out.update(adam_m=fu.m, adam_v=fu.v, adam_step=fu.step_count, hyper=fu.hyper)
    for n in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_adv", "b_ret", "b_epret", "b_done", "b_eplen", "b_outcome",
              "last_value", "obs"):
        out[n] = getattr(t, n)
    return out


def _same_bits(a, b):
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("N,group", ((1, False), (16, True)), ids=("n1", "n16_group"))
def test_pbt_trainer_without_exchange_is_the_population_trainer_bitwise(g, N, group):
    """fraction = 0: three iterations, an R = 0 exploit launch after each.  K = 3, EM = 64, n_steps = 2, batch 64: every
    minibatch is one wavefront per network, so the update itself is bitwise reproducible."""
    a = _trainer(g, g.PBTConfig(ready_every=1, fraction=0.0), N=N, group=group)
    b = _trainer(g, None, N=N, group=group)
    n = 3 * 2 * 64
    ha, hb = a.learn(n, log=None), b.learn(n, log=None)
    torch.cuda.synchronize()
    assert a.num_timesteps == b.num_timesteps == n and a.generation == 3
    sa, sb = _state(a), _state(b)
    for name in sa:
        assert _same_bits(sa[name], sb[name]), name
    recs = [h for h in ha if "exploit" in h]
    assert len(recs) == 9 and all(h["exploit"] is None for h in recs)
    assert len(ha) - len(recs) == len(hb) == 9


def test_pbt_trainer_refuses_members_with_their_own_gamma():
    """Nothing is launched: the rules are checked before the env is touched (a stub env: construction then gets as far as
    its missing reset())."""
    import types

    import gym_acas2d_amd as g
    venv = types.SimpleNamespace(dtype=torch.float32, n_traffic=1, obs_dim=8, num_envs=128, device="cpu")
    for f in ("gamma", "gae_lambda"):
        cfgs = [g.PPOConfig(n_steps=2, batch_size=64, **{f: v}) for v in (0.9, 0.95)]
        with pytest.raises(ValueError, match="%s.*not exchanged" % f):
            g.PBTTrainer(venv, cfgs, g.PBTConfig(ready_every=1))
    with pytest.raises(ValueError, match="2 x n_replace <= K"):
        g.PBTTrainer(venv, [g.PPOConfig(n_steps=2, batch_size=64)] * 2, g.PBTConfig(ready_every=1, fraction=1.0))
    with pytest.raises(AttributeError, match="reset"):
        g.PBTTrainer(venv, [g.PPOConfig(n_steps=2, batch_size=64)] * 2, g.PBTConfig(ready_every=1))


@pytest.mark.gpu
def test_pbt_trainer_exchange_equals_the_referee_on_a_snapshot(g):
    """K = 4, fraction 0.25, ready_every 1 (max_steps 15 < n_steps 24: every env ends an episode in the window)."""
    pbt = g.PBTConfig(ready_every=1, fraction=0.25, seed=77)
    t = _trainer(g, pbt, N=1, K=4, EM=64, T=24, B=512, max_steps=15)
    assert t.n_replace == 1 and t._fused_update is not None
    t.collect()
    # the window against what the parent's host path gathered for the same iteration
    w = {n: v.cpu().numpy() for n, v in t.window.items()}
    for k in range(4):
        r = torch.cat(t.ep_returns[k]).double().numpy()
        l, o = torch.cat(t.ep_lengths[k]).numpy(), torch.cat(t.ep_outcomes[k]).numpy()
        assert w["count"][k] == len(r) > 0 and w["steps"][k] == int(l.sum())
        assert list(w["outcomes"][k]) == [int((o == c).sum()) for c in range(4)]
        assert abs(w["score"][k] - r.mean()) <= 1e-6 * abs(r.mean())
    from gym_acas2d_amd.ppo import PopulationTrainer
    PopulationTrainer.update(t)                          # the parent's update alone: no exploit yet
    torch.cuda.synchronize()
    snap = {n: v.clone() for n, v in _state(t).items()}
    score, hyper0 = t.window["score"].cpu().numpy().copy(), t.hyper.cpu().numpy().copy()
    recs = t.exploit()
    torch.cuda.synchronize()
    lo, hi = np.full(8, -np.inf, F32), np.full(8, np.inf, F32)
    mask = 0
    for name in pbt.perturb:
        s = R.HYPER_SLOTS.index(name)
        mask |= 1 << s
        lo[s], hi[s] = pbt.bounds[name]
    d_ref, h_ref = R.exploit(score, hyper0, 1, 0, 77, mask, 0.8, 1.2, lo, hi)
    assert (d_ref != np.arange(4)).sum() == 1            # distinct scores: the worst member copies the best
    worst, best = int(np.argmin(score)), int(np.argmax(score))
    assert d_ref[worst] == best
    now = _state(t)
    sel = torch.as_tensor(d_ref.astype(np.int64), device=DEV)
    for name in list(t.policy_set.params) + ["adam_m", "adam_v", "adam_step"]:
        assert _same_bits(now[name], snap[name][sel]), name
    assert np.array_equal(now["hyper"].cpu().numpy().view(np.uint32), h_ref.view(np.uint32))
    assert not np.array_equal(h_ref[worst], hyper0[best])  # explored: the copied row was perturbed
    assert [r["exploit"] for r in recs] == [None if d_ref[k] == k else int(d_ref[k]) for k in range(4)]
    assert all(r["member"] == k and np.array_equal(np.asarray(r["hyper"], F32), h_ref[k]) for k, r in enumerate(recs))
    assert recs == t.history[-4:] and t.generation == 1
    assert int(t.window["count"].sum()) == 0 and bool(torch.isnan(t.window["score"]).all())
    # two further iterations: the copied member collects and updates like any other
    hist = t.learn(t.num_timesteps + 2 * 24 * 64, log=None)
    losses = [h for h in hist if "value_loss" in h]
    assert len(losses) == 8 and all(np.isfinite(h["value_loss"]) and np.isfinite(h["pg_loss"]) for h in losses)
    assert len([h for h in hist if "exploit" in h]) == 12 and t.generation == 3
    assert all(bool(torch.isfinite(p).all()) for p in t.policy_set.params.values())


@pytest.mark.gpu
def test_pbt_trainer_with_kernel_gae_is_the_torch_run_bitwise(g):
    pbt = g.PBTConfig(ready_every=1, fraction=0.25, seed=3)
    tk = _trainer(g, pbt, K=4, T=24, B=64, max_steps=15, gae="kernel", epochs=1)
    tt = _trainer(g, pbt, K=4, T=24, B=64, max_steps=15, gae=None, epochs=1)
    for t in (tk, tt):
        t.collect()
        t.update()
    torch.cuda.synchronize()
    sk, st = _state(tk), _state(tt)
    for name in sk:
        assert _same_bits(sk[name], st[name]), name
    assert [h["exploit"] for h in tk.history] == [h["exploit"] for h in tt.history]
    assert any(h["exploit"] is not None for h in tk.history)
