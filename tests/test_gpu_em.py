"""GPU: the transition statistics (hyg_tg_transition_stats through
hygeia_amd/em.py) against the numpy restatement tests/em_model.py, every
integer; their additivity; `hygeia fit_genome` end to end; and the statistics
of real launches' draws against the exact smoother's expectations.

Bar: exact wherever integers are compared. The kernel's tile is 256 sites, so
group beginnings sit at rows 255, 256, 257 as well as 63, 64, 65."""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_model as emm  # noqa: E402
from cli_trees import _write_chrom  # noqa: E402
from tg_exact_model import ExactModel, phantom_regime  # noqa: E402

K, U, T = 3, 3, 1000
MU, SIGMA = [0.15, 0.5, 0.85], [0.08, 0.12, 0.08]
THETA = np.array([0.3, -0.2, 0.1, 0.4, -0.5, 0.2] + [math.log(0.8 / 0.2), math.log(0.7 / 0.3), math.log(0.85 / 0.15)])
# holes: [60, 63), [215, 255), [457, 500), [800, 830); one-row groups at 63, 64, 255, 256; a group from row 0
SEG = [(0, 60), (63, 1), (64, 1), (65, 150), (255, 1), (256, 1), (257, 200), (500, 300), (830, 170)]
SHAPES = {50: (25, 2), 21: (7, 3), 275: (25, 11)}  # P: (B, seeds)
CASES = [(50, 3, 8), (50, 0, 4096), (21, 1, 8), (21, 3, 4096), (275, 3, 4096), (275, 1, 8)]  # (P, minimum_duration, dcap)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from hygeia_amd import _lib

    if _lib.load().hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _dev(a, dtype=torch.int16):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _paths(P):
    """[T][P] trajectories: legal paths of the model's prior, then per column
    class a duration offset modulo 2^16 (a fifth of the columns cross 32767 ->
    -32768 whenever a sojourn reaches 5 sites, another fifth -1 -> 0), merged
    stored as 3 in a third of the columns, and 6 % of the rows replaced by
    random, illegal words (any int16 duration, regimes up to 6, merged in
    {-2, 0, 1, 3})."""
    ex = ExactModel(K, MU, SIGMA, THETA, u=U, split_prob=0.05, merge_log_prob=math.log(0.2))
    merged, control, case = emm.sample_paths(ex, T, P, 100 + P)
    rng = np.random.default_rng(200 + P)
    off = np.where(np.arange(P) % 5 == 1, 32768 - 5, np.where(np.arange(P) % 5 == 3, 65536 - 5, 0))
    for st in (control, case):
        st[:, :, 0] = ((st[:, :, 0].astype(np.int64) + off[None, :]) & 0xffff).astype(np.uint16).view(np.int16)
    merged[:, np.arange(P) % 3 == 2] *= 3
    rows = rng.random(T) < 0.06
    n = int(rows.sum())
    merged[rows] = rng.choice(np.array([-2, 0, 1, 3], dtype=np.int16), (n, P))
    for st in (control, case):
        st[rows, :, 0] = rng.integers(-32768, 32768, (n, P))
        st[rows, :, 1] = rng.integers(0, 7, (n, P))
    for st in (control, case):
        d0, d1 = st[:-1, :, 0], st[1:, :, 0]
        assert ((d0 == 32767) & (d1 == -32768)).any() and ((d0 == -1) & (d1 == 0)).any()
    return merged, control, case


def _scatter(merged, control, case, B, S, seg, seed):
    """The trajectories of the groups `seg` as seed blocks placed in a shuffled
    order in one buffer, as hyg_tg_outputs holds them; every row that belongs
    to no group (the sites in no group are not in the buffer at all) holds a
    poison pattern that would count as a merged trial and a hazard event if it
    were read: (merged [rows][B], control, case [rows][B][2], block_rows)."""
    rng = np.random.default_rng(seed)
    rows = sum(r for _, r in seg) * S + 2 * len(seg) * S + 23
    m_b = np.full((rows, B), 1, dtype=np.int16)
    c_b = np.empty((rows, B, 2), dtype=np.int16)
    c_b[..., 0], c_b[..., 1] = 1, 1
    k_b = c_b.copy()
    k_b[..., 1] = 2
    starts, o = {}, 7
    for q in rng.permutation(len(seg) * S):
        g, s = divmod(int(q), S)
        starts[(g, s)] = o
        s0, nr = seg[g]
        m_b[o:o + nr] = merged[s0:s0 + nr, s * B:(s + 1) * B]
        c_b[o:o + nr] = control[s0:s0 + nr, s * B:(s + 1) * B]
        k_b[o:o + nr] = case[s0:s0 + nr, s * B:(s + 1) * B]
        o += nr + int(rng.integers(0, 3))  # poison rows between the blocks as well
    assert o <= rows and all(starts[(g, s)] + seg[g][1] <= rows for g in range(len(seg)) for s in range(S))
    return m_b, c_b, k_b, [[starts[(g, s)] for s in range(S)] for g in range(len(seg))]


@functools.lru_cache(maxsize=None)
def _buffers(P):
    B, S = SHAPES[P]
    m_b, c_b, k_b, block_rows = _scatter(*_paths(P), B, S, SEG, 300 + P)
    return _dev(m_b), _dev(c_b), _dev(k_b), block_rows


@functools.lru_cache(maxsize=None)
def _expected(P, u, dcap):
    return emm.transition_stats(*_paths(P), SEG, u, dcap)


def _same(got, want):
    for g, w, name in zip(got, want, ("table", "trials", "events")):
        assert g.dtype == np.int64 and g.shape == w.shape
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("P,u,dcap", CASES)
def test_kernel_equals_the_restatement(P, u, dcap):
    """1 000 sites in nine groups (SEG), P = 25 x 2, 7 x 3 (P does not divide
    the workgroup) and 25 x 11 (> 256), dcap 8 (the pooled last bin is by far
    the fullest) and 4096, minimum_duration 0, 1, 3."""
    from hygeia_amd import em

    B, S = SHAPES[P]
    want = _expected(P, u, dcap)
    table, trials, events = want
    assert (table > 0).all() and events.sum() > 0 and (events <= trials).all()
    assert trials.sum() < (T - len(SEG)) * P  # not every transition is a hazard trial
    if dcap == 8:
        assert trials[8] == trials.max() and 3 * trials[8] > trials.sum()
    else:
        assert np.count_nonzero(trials) > 30 and trials[1024:].sum() > 0  # the wrapped and random durations
    m, c, k, block_rows = _buffers(P)
    _same(em.transition_stats(m, c, k, B, SEG, block_rows, T, u, dcap), want)


def test_first_rows_and_uncovered_sites_count_nothing():
    """The same paths as one group differ (the group boundaries then are
    transitions), and groups of one row alone give zeros."""
    from hygeia_amd import em

    P, (B, S) = 50, SHAPES[50]
    one = emm.transition_stats(*_paths(P), [(0, T)], 3, 8)
    assert (one[0] != _expected(P, 3, 8)[0]).any()
    m, c, k, block_rows = _buffers(P)
    singles = [i for i, (_, n) in enumerate(SEG) if n == 1]
    got = em.transition_stats(m, c, k, B, [SEG[i] for i in singles], [block_rows[i] for i in singles], T, 3, 8)
    assert all(not a.any() for a in got)
    got = em.transition_stats(m, c, k, B, [], [], T, 3, 8)
    assert all(not a.any() for a in got)


def test_additivity_and_repeatability():
    """Two calls over two halves of the groups equal one call; a second
    identical call doubles every entry; two fresh calls give the same integers."""
    from hygeia_amd import em

    P, u, dcap = 275, 3, 4096
    B, S = SHAPES[P]
    m, c, k, block_rows = _buffers(P)
    want = _expected(P, u, dcap)
    stats = torch.zeros(em.stats_len(dcap), dtype=torch.int64, device="cuda:0")
    half = em.transition_stats(m, c, k, B, SEG[:5], block_rows[:5], T, u, dcap, stats=stats)
    assert 0 < half[1].sum() < want[1].sum()
    _same(em.transition_stats(m, c, k, B, SEG[5:], block_rows[5:], T, u, dcap, stats=stats), want)
    _same(em.transition_stats(m, c, k, B, SEG, block_rows, T, u, dcap, stats=stats), [2 * w for w in want])
    _same(em.split_stats(stats.cpu().numpy(), dcap), [2 * w for w in want])
    _same(em.transition_stats(m, c, k, B, SEG, block_rows, T, u, dcap), want)


# -------------------------------------------------------------- fit_genome
def _tree_bytes(root):
    out = {}
    for name in sorted(os.listdir(root)):
        with open(os.path.join(root, name), "rb") as fh:
            out[name] = fh.read()
    return out


def _read_tsv(path):
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[-1] == ""
    return [ln.split("\t") for ln in lines[:-1]]


def test_fit_genome_end_to_end(tmp_path, monkeypatch):
    """Two chromosomes of 600 sites, K = 3, M = 20, B = 25, seeds 0 and 5,
    segments of 250 with buffers of 30 (three tasks each), two iterations.
    Iteration 1's statistics are the restatement's on a stand-alone
    run_chains_host launch of the same tasks at the starting settings, its
    settings m_step of them; iteration 2's statistics those of a launch at
    these settings; a second run writes the same bytes."""
    from hygeia_amd import cli, em, two_group
    from hygeia_amd import synthetic as syn

    Kk, M, B, seeds, S, buf, dcap, u = 3, 20, 25, (0, 5), 250, 30, 64, 3
    root = str(tmp_path)
    chroms = (("21", 600, 0), ("X", 600, 1))
    for chrom, n, k in chroms:
        _write_chrom(root, chrom, n, k, K=Kk)
    mu, sg = syn.regime_params(Kk)
    start = dict(omega_case=0.6, merge_log_prob=math.log(0.3), split_prob=0.1)
    argv = ["fit_genome", "--chroms", "all", "--mu", ",".join(repr(float(x)) for x in mu), "--sigma",
            ",".join(repr(float(x)) for x in sg), "--segment_size", str(S), "--buffer_size", str(buf), "--seeds",
            "0,5", "--num_samples_backward", str(B), "--num_resampled_particles", str(M), "--iterations", "2",
            "--dcap", str(dcap), "--data_dir", str(tmp_path / "data"), "--single_group_dir", str(tmp_path / "sg"),
            "--results_dir", "res"] + [f"--{n}={v!r}" for n, v in start.items()]
    trees = []
    for d in ("a", "b"):
        os.makedirs(tmp_path / d)
        monkeypatch.chdir(tmp_path / d)
        assert cli.main(argv) == 0
        trees.append(_tree_bytes(str(tmp_path / d / "res")))
    assert trees[0] == trees[1]
    assert sorted(trees[0]) == ["fit_stats_1.npz", "fit_stats_2.npz", "fit_trace.tsv", "fitted_flags.txt"]
    res = tmp_path / "a" / "res"

    # the same tasks, laid out by hand
    mu32, sg32 = np.array(mu, dtype=np.float32), np.array(sg, dtype=np.float32)
    counts = {k: [] for k in ("mc", "tc", "mk", "tk")}
    chains, chain_model, tasks, thetas, out, site0, max_reads = [], [], [], [], 0, 0, 0
    for g, (chrom, n, k) in enumerate(chroms):
        d = syn.simulate(n, 2, 2, K=Kk, seed=60 + k, coverage=30.0)
        for key, name in (("mc", "meth_control"), ("tc", "tot_control"), ("mk", "meth_case"), ("tk", "tot_case")):
            counts[key].append(d[name].astype(np.float32))
        max_reads = max(max_reads, int(d["tot_control"].max()), int(d["tot_case"].max()))
        thetas.append(cli.control_theta(cli.read_theta(str(tmp_path / "sg"), chrom), Kk, chrom))
        for b in range(n // S + 1):
            (lo, hi), (r0, r1) = cli.segment_index(n, b, S, buf)
            begins = []
            for sd in seeds:
                chains.append((site0 + lo, hi - lo, sd, cli.chain_id(chrom, b), out))
                chain_model.append(g)
                begins.append(out)
                out += hi - lo
            tasks.append((g, lo, hi, r0, r1, begins))
        site0 += n
    counts = {k: np.concatenate(v) for k, v in counts.items()}
    assert len(chains) == 12

    def launch_stats(settings):
        models = two_group.genome_models(thetas, mu32, sg32, max_reads, [S + 2 * buf + 1] * 2, minimum_duration=u,
                                         num_resampled_ancestors=M, num_samples_backward=B, **settings)
        try:
            r = two_group.run_chains_host({"control": counts["mc"], "case": counts["mk"]},
                                          {"control": counts["tc"], "case": counts["tk"]}, models, chains, out,
                                          chain_model=chain_model)
        finally:
            for model in models:
                model.close()
        assert (r["status"] == 0).all()
        total = [np.zeros((2, 2), dtype=np.int64), np.zeros(dcap + 1, dtype=np.int64),
                 np.zeros(dcap + 1, dtype=np.int64)]
        for (g, lo, hi, r0, r1, begins) in tasks:  # a task's trimmed rows, its seeds side by side
            by_site = [np.concatenate([r[name][o + r0:o + r1] for o in begins], axis=1)
                       for name in ("merged", "control", "case")]
            for acc, part in zip(total, emm.transition_stats(*by_site, [(0, r1 - r0)], u, dcap)):
                acc += part
        return total, math.fsum(r["log_z"].tolist())

    trace = _read_tsv(res / "fit_trace.tsv")
    assert tuple(trace[0]) == em.TRACE_COLUMNS and len(trace) == 3
    settings = start
    for it in (1, 2):
        want, sum_log_z = launch_stats(settings)
        with np.load(res / f"fit_stats_{it}.npz") as z:
            _same([z["table"], z["trials"], z["events"]], want)
        assert want[0].sum() > 1000 and want[2].sum() > 0
        new, rec = em.m_step(want, settings, u, 2.0, em.SETTINGS)
        row = trace[it]
        assert row[0] == str(it)
        assert row[1:4] == [repr(float(settings[n])) for n in em.SETTINGS]
        assert row[4:7] == [repr(float(new[n])) for n in em.SETTINGS]
        assert row[7:11] == [str(int(v)) for v in want[0].reshape(-1)]
        assert row[11:13] == [str(int(want[1].sum())), str(int(want[2].sum()))]
        assert row[13:15] == [repr(float(rec["q_before"])), repr(float(rec["q_after"]))]
        assert abs(float(row[15]) - sum_log_z) <= 1e-9 * abs(sum_log_z)
        assert new != settings
        settings = new
    with open(res / "fitted_flags.txt") as fh:
        assert fh.read() == em.serialize_settings(settings)
    # the flags file feeds `infer`'s parser as it is
    f = cli.parse_flags(open(res / "fitted_flags.txt").read().split("\n"))
    assert [f[n] for n in em.SETTINGS] == [settings[n] for n in em.SETTINGS]


# ------------------------------------------- draws against the exact smoother
def test_statistics_of_the_draws_match_the_exact_smoother(oracle):
    """The pattern of tests/test_gpu_tg_exact.py: a 12-site K = 3, u = 2 chain,
    weak data, 40 seeds x B = 25 backward draws in one launch. Per trajectory
    the six aggregate statistics (the four table cells, total trials, total
    events); the mean of each lies within 5 empirical standard errors of the
    expectation under ExactModel's pairwise smoothing marginals (given each
    seed's phantom regime). Seeds are fixed, so the test is deterministic.

    M = 256, the largest the kernels run. At 12 sites that does not keep every
    particle: this chain has 2, 2, 18, 50, 226 and then more than 256 finite
    particles at steps 0 to 5, so from the sixth step on the filter resamples
    optimally and the draws are the particle smoother's, not exact draws. (The
    keep-all regime ends at 6 sites for K = 3, u = 2, where the events are too
    rare for an empirical standard error over 1 000 draws.) The same run on
    the CPU oracle gives |z| <= 0.54 for the six means."""
    from test_tg_exact import _problem

    from hygeia_amd import em, two_group

    Kk, Tt, u, M, B, cid, seeds = 3, 12, 2, 256, 25, 7, list(range(40))
    p, ex, E, E_ex = _problem(oracle, Kk, Tt, 31, M=M, B=B, cov=2, u=u, S=2)
    dev = torch.device("cuda", 0)
    model = two_group.CaseControlModel([p.mu[i] for i in range(Kk)], [p.sigma[i] for i in range(Kk)],
                                       [p.theta[i] for i in range(p.theta_len)], minimum_duration=u,
                                       num_resampled_ancestors=M, num_samples_backward=B, max_total_reads=64,
                                       max_duration=Tt + 5)
    dc = two_group.DeviceChains(model, [(0, Tt, s, cid, i * Tt) for i, s in enumerate(seeds)], Tt * len(seeds),
                                device=dev)
    dc.run(torch.from_numpy(np.ascontiguousarray(E)).to(dev))
    torch.cuda.synchronize()
    assert (dc.status.cpu().numpy() == 0).all()
    agg = lambda st: np.array([st[0][0, 0], st[0][0, 1], st[0][1, 0], st[0][1, 1], st[1].sum(), st[2].sum()],  # noqa: E731
                              dtype=np.float64)
    total = agg(em.transition_stats(dc.merged, dc.control, dc.case, B, [(0, Tt)], [[i * Tt for i in range(len(seeds))]],
                                    Tt, u, Tt + 1))
    mg, ct, cs = dc.merged.cpu().numpy(), dc.control.cpu().numpy(), dc.case.cpu().numpy()
    exact, deviations, per_traj = {}, [], np.zeros(6)
    for i, s in enumerate(seeds):
        r_ph = phantom_regime(oracle, s, cid, Kk)
        if r_ph not in exact:
            exact[r_ph] = agg(emm.expected_stats(ex.forward_backward(E_ex, r_ph)[3], u, Tt + 1))
        for b in range(B):
            o = slice(i * Tt, (i + 1) * Tt)
            a = agg(emm.transition_stats(mg[o, b:b + 1], ct[o, b:b + 1], cs[o, b:b + 1], [(0, Tt)], u, Tt + 1))
            per_traj += a
            deviations.append(a - exact[r_ph])
    np.testing.assert_array_equal(total, per_traj)  # the kernel's sums are the trajectories' own
    assert len(exact) >= 2
    d = np.array(deviations)
    mean, se = d.mean(axis=0), d.std(axis=0, ddof=1) / math.sqrt(len(d))
    print("mean deviation", mean, "standard error", se, "z", mean / se)
    assert (se > 0).all()
    assert (np.abs(mean) <= 5 * se).all(), (mean, se)
