"""`hygeia estimate_parameters_and_regimes` on the MI355X path: a drop-in for the
single-group container's R script src/single_group/bin/estimate_parameters_and_regimes,
which the two-group pipeline's step 2 runs per chromosome
(modules/two_group/2_estimate_parameters_and_regimes.nf:38-52) to produce the
theta_{chrom}.csv.gz that `hygeia infer` reads.

Same flags (R argparser spellings and defaults, :10-204), same inputs and
outputs (:216-379); the engine is the C ABI's single-group SMC with optimal
finite-state resampling, online marginal smoothing and (--estimate_parameters)
online parameter estimation (hyg_sg_run_chain_host[_pe], the HIP kernels of
libhygeia_amd.so; no CPU path). Reproduced quirks:

- read_csv with a header (input_output_functions.R:10-20): the pipeline's count
  files have none, so their first CpG site becomes the header and is dropped;
- convert_model_parameters_to_theta takes p[p != -1] column-major
  (model_functions.R:62-76) while the engine reads theta blocks as rows: a p
  from --p_input_csv_file enters transposed, and convert_theta_to_model_parameters
  (:78-111) writes p back row-major;
- the default p (:243-247) has 1/5 off the diagonal whatever the number of
  regimes (the engine's softmax normalises the rows);
- --estimate_parameters starts theta from the prior, K^2 standard normal draws
  (sampleFromParameterPriorCpp, singleGroup.cpp:18-35, singleGroup.h:480-483),
  not from --p / --omega;
- --randomise_rng_seed defaults to TRUE (:191-197): runs are not reproducible
  unless it is FALSE (then --rng_seed seeds every draw);
- the regimes CSV holds R format(scientific = FALSE) strings (:326-338):
  fixed notation, 7 significant digits, one width and one number of decimals
  per column (`r_format_column`).

Parity unpinned where R is the reference: R's RNG (arma::randn / the engine's
streams) is not reproduced, and readr's number writer is replaced by Python's
shortest round-trip text (the same values), except in the theta file, written
with 17 significant digits in exponent form so that `hygeia infer`'s pandas
parser reads it within 3 ulp (write_vector).

`hygeia estimate_genome` (estimate_genome, run_engine_many) is the same command
over chromosomes: every chromosome's chain in one multi-model launch
(hyg_sg_run_chains_host_multi), each under its own model, per chromosome the
files of the single command. No reference counterpart: the pipeline starts a
process per chromosome.

`hygeia sg_log_z` (sg_log_z, filter_many) scores what those commands choose:
log Z of every chromosome under a grid of parameter sets, minimum durations and
seeds, from forward-only launches (hyg_sg_filter_chains_host_multi,
hyg_sg_trace_chains_host_multi), with the filter trace on request. No reference
counterpart either: the reference's engine reports no likelihood.

`hygeia sg_sample_genome` (sg_sample_genome, sample_many) draws joint
segmentations, whole paths (d_t, r_t) per chromosome and seed, by backward
simulation from the particle history of a forward-only launch
(hyg_sg_sample_chains_host_multi), and can write them as the matrices `hygeia
get_change_points` reads. No reference counterpart: its engine stops at marginals.
"""
from __future__ import annotations

import gzip
import math
import os
import sys
from typing import Dict, Sequence

import numpy as np

from .cli import FlagError, GenomeInputError

# (name, kind, default) in the R script's definition order
# (bin/estimate_parameters_and_regimes:12-204); kinds: str, int, double,
# logical (a value: TRUE / FALSE / T / F ...), flag (no value: TRUE if present)
FLAGS = [
    ("mu", "str", "0.99,0.01,0.80,0.20,0.50,0.50"),
    ("sigma", "str", "0.05,0.05,0.20,0.20,0.20,0.2886751"),
    ("u", "int", 2),
    ("kappa", "str", "2,2,2,2,2,2"),
    ("omega", "str", "0.995,0.975,0.950,0.925,0.900,0.900"),
    ("p_input_csv_file", "str", None),
    ("kappa_input_csv_file", "str", None),
    ("omega_input_csv_file", "str", None),
    ("n_methylated_reads_csv_file", "str", None),
    ("genomic_positions_csv_file", "str", None),
    ("n_total_reads_csv_file", "str", None),
    ("regime_probabilities_csv_file", "str", None),
    ("theta_trace_csv_file", "str", None),
    ("omega_csv_file", "str", "omega.csv"),
    ("kappa_csv_file", "str", "kappa.csv"),
    ("p_csv_file", "str", "p.csv"),
    ("theta_file", "str", "p.csv"),
    ("is_kappa_fixed", "logical", True),
    ("n_particles", "int", 250),
    ("estimate_regime_probabilities", "flag", False),
    ("estimate_parameters", "flag", False),
    ("epsilon", "double", 0.01),
    ("normalise_gradients", "logical", False),
    ("use_adam", "logical", True),
    ("n_steps_without_parameter_update", "int", 200),
    ("learning_rate_exponent", "double", 0.1),
    ("learning_rate_factor", "double", 0.01),
    ("root_dir", "str", "./src/r"),
    ("randomise_rng_seed", "logical", True),
    ("rng_seed", "int", -73),
]

_TRUE = {"TRUE", "T", "true", "True"}
_FALSE = {"FALSE", "F", "false", "False"}


def parse_flags(argv: Sequence[str], flags=None) -> Dict[str, object]:
    """argparser-style parsing: `--name value` or `--name=value`; logical values
    as R's as.logical reads them; flags take no value. `flags`: the
    specification, FLAGS unless given."""
    flags = FLAGS if flags is None else flags
    spec = {n: (k, d) for n, k, d in flags}
    out = {n: d for n, _, d in flags}
    argv = list(argv)
    i = 0
    while i < len(argv):
        a = argv[i]
        if not a.startswith("--"):
            raise FlagError(f"unexpected argument {a!r}")
        name, eq, val = a[2:].partition("=")
        if name not in spec:
            raise FlagError(f"unknown argument --{name}")
        kind = spec[name][0]
        if kind == "flag":
            if eq:
                raise FlagError(f"--{name} is a flag and takes no value")
            out[name] = True
            i += 1
            continue
        if not eq:
            if i + 1 >= len(argv):
                raise FlagError(f"--{name} needs a value")
            val = argv[i + 1]
            i += 2
        else:
            i += 1
        try:
            if kind == "int":
                out[name] = parse_int(val)
            elif kind == "double":
                out[name] = float(val)
            elif kind == "logical":
                if val in _TRUE:
                    out[name] = True
                elif val in _FALSE:
                    out[name] = False
                else:
                    raise ValueError("not a logical")
            else:
                out[name] = val
        except ValueError as e:
            raise FlagError(f"invalid value for --{name}: {val!r} ({e})")
    return out


def parse_int(val: str) -> int:
    """as.integer of a flag's text: "3" and "3.0" read as 3. Integer text is
    read exactly (a 64-bit seed from rng_seeds.csv does not fit a double); only
    other forms go through a double."""
    try:
        return int(str(val).strip())
    except ValueError:
        v = float(val)
        if v != int(v):
            raise ValueError("not an integer")
        return int(v)


def _numbers(s: str) -> np.ndarray:
    return np.array([float(x) for x in str(s).split(",") if x.strip() != ""], dtype=np.float64)


# ------------------------------------------------------------------- inputs
def _open(path: str, mode: str = "rt"):
    return gzip.open(path, mode) if path.endswith(".gz") else open(path, mode)


def read_csv_matrix(path: str) -> np.ndarray:
    """readr::read_csv(file) as a numeric matrix (read_from_csv_file,
    input_output_functions.R:10-20): the FIRST LINE IS THE HEADER, whatever it
    holds, so a headerless count file loses its first CpG site (Appendix B.3)."""
    with _open(path) as fh:
        header = fh.readline()
        ncol = len(header.rstrip("\r\n").split(","))
        rows = fh.read()
    if not rows.strip():
        return np.zeros((0, ncol))
    a = np.loadtxt(rows.splitlines(), delimiter=",", dtype=np.float64, ndmin=2)
    if a.shape[1] != ncol:
        raise ValueError(f"{path}: {a.shape[1]} columns, header has {ncol}")
    return a


def default_p(K: int) -> np.ndarray:
    """The initial transition matrix of the R script (:243-247):
    matrix(c(rep(c(0, rep(1/5, K)), K - 1), 0), K, K), filled column-major."""
    v = np.concatenate([np.tile(np.concatenate([[0.0], np.full(K, 1 / 5)]), K - 1), [0.0]])
    return v.reshape(K, K, order="F")


def theta_from_model(p: np.ndarray, omega: np.ndarray, kappa=None) -> np.ndarray:
    """convert_model_parameters_to_theta (model_functions.R:65-78):
    diag(p) <- -1; c(log(p[p != -1]), logit(omega)) -- p[p != -1] in R's
    column-major order -- and log(kappa) appended when kappa is estimated
    (kappa given)."""
    p = np.array(p, dtype=np.float64)
    np.fill_diagonal(p, -1.0)
    flat = p.flatten(order="F")
    off = flat[flat != -1.0]
    with np.errstate(divide="ignore"):
        parts = [np.log(off), np.log(omega) - np.log(1.0 - omega)]
        if kappa is not None:
            parts.append(np.log(np.asarray(kappa, dtype=np.float64)))
        return np.concatenate(parts)


def model_from_theta(theta: np.ndarray, K: int):
    """convert_theta_to_model_parameters (model_functions.R:81-111): row r of p
    = exp(normalise_exp(theta block r)) off the diagonal (row-major), omega =
    inverse_logit(theta[K(K-1):K^2]) and, when theta carries the K log kappa
    entries (kappa estimated), kappa = exp(theta[K^2:K(K+1)]) (else None)."""
    p = np.zeros((K, K))
    for r in range(K):
        blk = theta[r * (K - 1):(r + 1) * (K - 1)]
        m = blk.max()
        lz = m + math.log(np.exp(blk - m).sum())
        p[r, [c for c in range(K) if c != r]] = np.exp(blk - lz)
    omega = 1.0 / (1.0 + np.exp(-theta[K * (K - 1):K * K]))
    kappa = np.exp(theta[K * K:K * (K + 1)]) if theta.shape[0] >= K * (K + 1) else None
    return p, omega, kappa


# ------------------------------------------------------------------ outputs
def r_format_column(x: np.ndarray, digits: int = 7) -> np.ndarray:
    """R's format(x, scientific = FALSE) of a double vector (formatReal in fixed
    notation): every element needs the fewest significant digits (<= `digits`)
    that show it to `digits` significant digits; the column takes the largest
    number of decimals any element needs and the widest integer part, and every
    element is printed "%*.*f" with that width and those decimals (right
    aligned, spaces). Returns an array of str. (R's own digit search uses long
    double arithmetic; here it is Python's correctly rounded '%.6e', so a value
    within an ulp of a rounding tie may choose one digit differently: parity
    unpinned, R is absent.)"""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return np.array([], dtype=str)
    fin = np.isfinite(x)
    rgt, left = 0, 1
    # distinct values decide the column's decimals (a column of probabilities or
    # positions has far fewer distinct values than rows)
    for v in np.unique(x[fin]):
        if v == 0.0:
            continue
        m, e = ("%.*e" % (digits - 1, abs(v))).split("e")
        kp = int(e)
        sig = len(m.replace(".", "").rstrip("0")) or 1
        rgt = max(rgt, sig - kp - 1)
        left = max(left, kp + 1)
    neg = bool(np.any(x[fin] < 0))
    out = np.array(["%.*f" % (rgt, v) for v in x.tolist()], dtype=object)
    width = max(len(s) for s in out) if out.size else 0
    width = max(width, neg + left + rgt + (rgt != 0))
    return np.array([s.rjust(width) for s in out])


def _shortest(v: float) -> str:
    """A double as the shortest text that reads back to the same value."""
    if v == int(v) and abs(v) < 1e15:
        return str(int(v))
    return repr(float(v))


def write_csv(path: str, header: Sequence[str], columns: Sequence[Sequence[str]], level: int = 6) -> None:
    """readr::write_csv of string columns (gzip by extension, as readr)."""
    body = "\n".join(",".join(row) for row in zip(*columns))
    text = ",".join(header) + "\n" + (body + "\n" if body else "")
    with (gzip.open(path, "wt", compresslevel=level) if path.endswith(".gz") else open(path, "w")) as fh:
        fh.write(text)


def write_vector(path: str, name: str, values: Sequence[float], exp17: bool = False) -> None:
    """write_to_csv_file(tibble(name = values)) (input_output_functions.R:4-7).
    exp17: 17 significant digits in exponent form ('%.16e'), which pandas'
    default parser -- `hygeia infer` reads the theta file with it, as
    run_inference_two_groups.py:76-79 does -- reads within 3 ulp; the shortest
    text of a small value ('0.00123...') has up to 21 mantissa characters, of
    which it keeps 17 (errors of thousands of ulp, tests/test_single_group_cli.py)."""
    write_csv(path, [name], [["%.16e" % v if exp17 else _shortest(v) for v in values]])


def write_theta_trace(path: str, theta_rows: np.ndarray, n_sites: int, every: int) -> None:
    """The thetaEstimates of every SMC step (OnlineParameterEstimation.h:42-61:
    theta_0 at t = 0, then theta after step t's update, which changes it only
    when t % every == 0), columns theta_1 .. theta_dim: row t is the engine's
    row t // every. Each distinct row is formatted once and repeated."""
    dim = theta_rows.shape[1]
    head = (",".join(f"theta_{j + 1}" for j in range(dim)) + "\n").encode()
    opener = gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")
    with opener as fh:
        fh.write(head)
        for i in range(theta_rows.shape[0]):
            reps = min(every, n_sites - i * every) if i > 0 else min(every, n_sites)
            if reps <= 0:
                break
            line = (",".join(_shortest(v) for v in theta_rows[i].tolist()) + "\n").encode()
            fh.write(line * reps)


def write_regimes(path: str, positions: np.ndarray, probs: np.ndarray) -> None:
    """regimes CSV (:326-338): genomic_position, regime_1 .. regime_K, each column
    R format(scientific = FALSE) text."""
    K = probs.shape[1]
    cols = [r_format_column(positions)] + [r_format_column(probs[:, r]) for r in range(K)]
    write_csv(path, ["genomic_position"] + [f"regime_{r + 1}" for r in range(K)], cols)


# ------------------------------------------------------------------- engine
def run_engine(L, K: int, u: int, alpha, beta, kappa, theta_init, epsilon: float, n_particles: int,
               meth: np.ndarray, tot: np.ndarray, seed: int, chain_id: int, estimate_parameters: bool, pe_flags=None,
               is_kappa_fixed: bool = True):
    """runOnlineCombinedInferenceCpp (singleGroup.cpp:76-189) through the C ABI:
    regime probabilities [T][K] and, with parameter estimation, the engine's
    theta rows [1 + (T - 1) / every][dim] (dim = K^2, or K (K + 1) with kappa
    estimated: then theta_init carries log kappa and `kappa` is unused, as
    vartheta has no kappa, model_functions.R:48-54)."""
    import ctypes as C

    from . import _lib

    dim = K * K if is_kappa_fixed else K * (K + 1)
    if len(theta_init) != dim:
        raise ValueError(f"theta has {len(theta_init)} entries, the model {dim}")
    p = _lib.SgParams()
    L.hyg_sg_params_default(C.byref(p))
    p.n_regimes, p.minimum_duration, p.num_particles_max = K, int(u), int(n_particles)
    p.resample_type, p.is_kappa_fixed, p.theta_len = 2, int(bool(is_kappa_fixed)), dim
    for r in range(K):
        p.alpha[r], p.beta[r] = float(alpha[r]), float(beta[r])
        p.kappa[r] = float(kappa[r]) if is_kappa_fixed else 0.0
    for i, v in enumerate(theta_init):
        p.theta[i] = float(v)
    p.epsilon = float(epsilon)
    T, S = tot.shape
    meth = np.ascontiguousarray(meth, dtype=np.uint16)
    tot = np.ascontiguousarray(tot, dtype=np.uint16)
    h = C.c_void_p()
    _lib.check(L.hyg_sg_model_create(C.byref(p), max(int(tot.max(initial=0)), 1), T + 10, C.byref(h)))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        probs = np.empty((T, K), np.float64)
        if not estimate_parameters:
            _lib.check(L.hyg_sg_run_chain_host(h, ptr(meth), ptr(tot), S, T, seed, chain_id, ptr(probs)))
            return probs, None
        pe = _lib.SgPeParams()
        L.hyg_sg_pe_params_default(C.byref(pe))
        pe.use_adam = int(pe_flags["use_adam"])
        pe.normalise_gradients = int(pe_flags["normalise_gradients"])
        pe.n_steps_without_update = int(pe_flags["n_steps_without_parameter_update"])
        pe.learning_rate_exponent = float(pe_flags["learning_rate_exponent"])
        pe.learning_rate_factor = float(pe_flags["learning_rate_factor"])
        ch = _lib.SgChain(0, T, 0, seed, chain_id, 0)
        rows = int(L.hyg_sg_pe_theta_rows(C.byref(ch), 1, pe.n_steps_without_update))
        theta = np.empty((rows, dim), np.float64)
        _lib.check(L.hyg_sg_run_chain_host_pe(h, C.byref(pe), ptr(meth), ptr(tot), S, T, seed, chain_id, ptr(probs),
                                              ptr(theta)))
        return probs, theta
    finally:
        L.hyg_sg_model_destroy(h)


def run_engine_many(L, K: int, u: int, alpha, beta, epsilon: float, n_particles: int, tasks,
                    estimate_parameters: bool, pe_flags=None, is_kappa_fixed: bool = True):
    """`run_engine` for a list of tasks in ONE launch
    (hyg_sg_run_chains_host_multi), each chain under its own model. A task is a
    dict with `meth` / `tot` [T][S], `theta_init`, `kappa`, `seed`, `chain_id`
    and optionally `epsilon` (else the shared one). Returns, in task order, what
    `run_engine` returns for each task alone: (probs, theta rows or None), bit
    for bit. The chains are handed over longest first: a launch that exceeds
    the device's chains per batch is split in the order given, and a batch lasts
    as long as its longest chain (the results do not depend on the order)."""
    import ctypes as C

    from . import _lib

    n = len(tasks)
    if n < 1:
        return []
    dim = K * K if is_kappa_fixed else K * (K + 1)
    S = tasks[0]["tot"].shape[1]
    for t in tasks:
        if len(t["theta_init"]) != dim:
            raise ValueError(f"theta has {len(t['theta_init'])} entries, the model {dim}")
        if t["tot"].ndim != 2 or t["tot"].shape != t["meth"].shape or t["tot"].shape[1] != S:
            raise ValueError("the tasks' count arrays disagree on their shape or their samples")
    order = sorted(range(n), key=lambda i: -tasks[i]["tot"].shape[0])
    lens = [tasks[i]["tot"].shape[0] for i in order]
    max_reads = max(max(int(t["tot"].max(initial=0)) for t in tasks), 1)
    meth = np.ascontiguousarray(np.concatenate([tasks[i]["meth"] for i in order]), dtype=np.uint16)
    tot = np.ascontiguousarray(np.concatenate([tasks[i]["tot"] for i in order]), dtype=np.uint16)
    total = int(sum(lens))
    handles = []
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        for i in order:
            t = tasks[i]
            p = _lib.SgParams()
            L.hyg_sg_params_default(C.byref(p))
            p.n_regimes, p.minimum_duration, p.num_particles_max = K, int(u), int(n_particles)
            p.resample_type, p.is_kappa_fixed, p.theta_len = 2, int(bool(is_kappa_fixed)), dim
            for r in range(K):
                p.alpha[r], p.beta[r] = float(alpha[r]), float(beta[r])
                p.kappa[r] = float(t["kappa"][r]) if is_kappa_fixed else 0.0
            for j, v in enumerate(t["theta_init"]):
                p.theta[j] = float(v)
            p.epsilon = float(t.get("epsilon", epsilon))
            h = C.c_void_p()
            _lib.check(L.hyg_sg_model_create(C.byref(p), max_reads, t["tot"].shape[0] + 10, C.byref(h)))
            handles.append(h)
        models = (C.c_void_p * n)(*[h.value for h in handles])
        chain_model = (C.c_int32 * n)(*range(n))
        chains = (_lib.SgChain * n)()
        begin = 0
        for k, i in enumerate(order):
            chains[k] = _lib.SgChain(begin, lens[k], 0, int(tasks[i]["seed"]), int(tasks[i]["chain_id"]), begin)
            begin += lens[k]
        probs = np.empty((total, K), np.float64)
        status = np.zeros(n, np.int32)
        pe, theta, rows = None, None, [0] * n
        if estimate_parameters:
            pe = _lib.SgPeParams()
            L.hyg_sg_pe_params_default(C.byref(pe))
            pe.use_adam = int(pe_flags["use_adam"])
            pe.normalise_gradients = int(pe_flags["normalise_gradients"])
            pe.n_steps_without_update = int(pe_flags["n_steps_without_parameter_update"])
            pe.learning_rate_exponent = float(pe_flags["learning_rate_exponent"])
            pe.learning_rate_factor = float(pe_flags["learning_rate_factor"])
            if pe.n_steps_without_update < 1:
                raise ValueError("n_steps_without_parameter_update < 1")
            rows = [1 + (T - 1) // pe.n_steps_without_update for T in lens]
            theta = np.empty((sum(rows), dim), np.float64)
        _lib.check(L.hyg_sg_run_chains_host_multi(
            models, n, C.byref(pe) if pe is not None else None, ptr(meth), ptr(tot), S, total, chains, chain_model, n,
            total, ptr(probs), ptr(theta) if theta is not None else None, ptr(status)))
    finally:
        for h in handles:
            L.hyg_sg_model_destroy(h)
    out = [None] * n
    begin = row = 0
    for k, i in enumerate(order):
        if status[k] != _lib.HYG_OK:
            raise _lib.HygError(int(status[k]), f"task {i}: " + (
                "pending smoothing times exceeded psi_capacity, or a sojourn outgrew the hazard rows"
                if status[k] == _lib.HYG_ENOMEM else "all particle weights became -inf"))
        out[i] = (probs[begin:begin + lens[k]].copy(),
                  theta[row:row + rows[k]].copy() if theta is not None else None)
        begin += lens[k]
        row += rows[k]
    return out


def filter_many(L, K: int, u: int, alpha, beta, n_particles: int, tasks, trace=None, is_kappa_fixed: bool = True):
    """The forward recursion alone for a list of tasks in ONE forward-only
    launch (hyg_sg_filter_chains_host_multi, with `trace`
    hyg_sg_trace_chains_host_multi): no smoothing, no regime tracks. The tasks
    are those of `run_engine_many` with a theta per task (`theta_init`, here the
    parameters the chain runs under). Returns, in task order, a dict with
    `log_z` (the SMC estimate of log p(y), bit for bit the log-sum-exp of the
    last step's unnormalised log-weights of the full launch's chain), `status`
    (HYG_OK or HYG_ENUMERIC; then log_z is -inf), `n_particles` and, with
    `trace`, the filter trace `log_z_t` [T], `regime_probs` [T][K] and
    `cp_probs` [T]. Tasks that name the same `tot` array share one copy of the
    counts, tasks with the same parameters and length one model."""
    return _forward_many(L, K, u, alpha, beta, n_particles, tasks, trace, is_kappa_fixed, None)


def sample_many(L, K: int, u: int, alpha, beta, n_particles: int, tasks, n_trajectories: int,
                is_kappa_fixed: bool = True):
    """Joint segmentations by backward simulation for a list of tasks in ONE
    launch pair (hyg_sg_sample_chains_host_multi: the history build of the
    forward-only launch, then the sampler). Tasks and grouping are
    `filter_many`'s. Returns, in task order, a dict with `paths` int16
    [T][n_trajectories][2] = (d mod 2^16, r) per site and trajectory (-1 for a
    chain that ended in HYG_ENUMERIC), `log_z` and `status`."""
    if not 1 <= int(n_trajectories) <= 1024:
        raise ValueError(f"n_trajectories must be in [1, 1024], got {n_trajectories}")
    return _forward_many(L, K, u, alpha, beta, n_particles, tasks, None, is_kappa_fixed, int(n_trajectories))


def _forward_many(L, K: int, u: int, alpha, beta, n_particles: int, tasks, trace, is_kappa_fixed: bool,
                  n_trajectories):
    """`filter_many` (n_trajectories None) and `sample_many`: one grouping, one
    set of models, one host entry."""
    import ctypes as C

    from . import _lib

    n = len(tasks)
    if n < 1:
        return []
    dim = K * K if is_kappa_fixed else K * (K + 1)
    S = tasks[0]["tot"].shape[1]
    for t in tasks:
        if len(t["theta_init"]) != dim:
            raise ValueError(f"theta has {len(t['theta_init'])} entries, the model {dim}")
        if t["tot"].ndim != 2 or t["tot"].shape != t["meth"].shape or t["tot"].shape[1] != S:
            raise ValueError("the tasks' count arrays disagree on their shape or their samples")
    order = sorted(range(n), key=lambda i: -tasks[i]["tot"].shape[0])
    lens = [tasks[i]["tot"].shape[0] for i in order]
    max_reads = max(max(int(t["tot"].max(initial=0)) for t in tasks), 1)
    # the counts of every distinct data set once, in the order first met
    site_of, parts_m, parts_t, total = {}, [], [], 0
    for i in order:
        key = (id(tasks[i]["tot"]), id(tasks[i]["meth"]))
        if key not in site_of:
            site_of[key] = total
            parts_m.append(tasks[i]["meth"])
            parts_t.append(tasks[i]["tot"])
            total += tasks[i]["tot"].shape[0]
    meth = np.ascontiguousarray(np.concatenate(parts_m), dtype=np.uint16)
    tot = np.ascontiguousarray(np.concatenate(parts_t), dtype=np.uint16)
    handles, model_of = [], {}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    try:
        cm = []
        for i in order:
            t = tasks[i]
            theta = np.asarray(t["theta_init"], np.float64)
            kappa = np.asarray(t["kappa"], np.float64)
            key = (theta.tobytes(), kappa.tobytes(), t["tot"].shape[0])
            if key not in model_of:
                p = _lib.SgParams()
                L.hyg_sg_params_default(C.byref(p))
                p.n_regimes, p.minimum_duration, p.num_particles_max = K, int(u), int(n_particles)
                p.resample_type, p.is_kappa_fixed, p.theta_len = 2, int(bool(is_kappa_fixed)), dim
                for r in range(K):
                    p.alpha[r], p.beta[r] = float(alpha[r]), float(beta[r])
                    p.kappa[r] = float(kappa[r]) if is_kappa_fixed else 0.0
                for j, v in enumerate(theta):
                    p.theta[j] = float(v)
                h = C.c_void_p()
                _lib.check(L.hyg_sg_model_create(C.byref(p), max_reads, t["tot"].shape[0] + 10, C.byref(h)))
                model_of[key] = len(handles)
                handles.append(h)
            cm.append(model_of[key])
        models = (C.c_void_p * len(handles))(*[h.value for h in handles])
        chain_model = (C.c_int32 * n)(*cm)
        chains = (_lib.SgChain * n)()
        row = 0
        for k, i in enumerate(order):
            begin = site_of[(id(tasks[i]["tot"]), id(tasks[i]["meth"]))]
            chains[k] = _lib.SgChain(begin, lens[k], 0, int(tasks[i]["seed"]), int(tasks[i]["chain_id"]), row)
            row += lens[k]
        log_z = np.empty(n, np.float64)
        npart = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        zt = rp = cp = paths = None
        if n_trajectories is not None:
            paths = np.full((row, n_trajectories, 2), -1, np.int16)
            _lib.check(L.hyg_sg_sample_chains_host_multi(models, len(handles), ptr(meth), ptr(tot), S, total, chains,
                                                         chain_model, n, n_trajectories, row, ptr(paths), ptr(log_z),
                                                         ptr(status)))
        elif trace:
            zt, rp, cp = np.empty(row, np.float64), np.empty((row, K), np.float64), np.empty(row, np.float64)
            _lib.check(L.hyg_sg_trace_chains_host_multi(models, len(handles), ptr(meth), ptr(tot), S, total, chains,
                                                        chain_model, n, row, ptr(zt), ptr(rp), ptr(cp), ptr(log_z),
                                                        None, None, ptr(npart), ptr(status)))
        else:
            _lib.check(L.hyg_sg_filter_chains_host_multi(models, len(handles), ptr(meth), ptr(tot), S, total, chains,
                                                         chain_model, n, ptr(log_z), None, None, ptr(npart),
                                                         ptr(status)))
    finally:
        for h in handles:
            L.hyg_sg_model_destroy(h)
    out = [None] * n
    row = 0
    for k, i in enumerate(order):
        o = {"log_z": float(log_z[k]), "status": int(status[k]), "n_particles": int(npart[k])}
        if paths is not None:
            del o["n_particles"]
            o["paths"] = paths[row:row + lens[k]].copy()
        if trace:
            o.update(log_z_t=zt[row:row + lens[k]].copy(), regime_probs=rp[row:row + lens[k]].copy(),
                     cp_probs=cp[row:row + lens[k]].copy())
        out[i] = o
        row += lens[k]
    return out


def _known_parameters(f):
    """get_known_parameters (model_functions.R:36-59) from the flags: K, whether
    kappa is fixed, and the Beta parameters by moments. Shared by `main` and
    `estimate_genome` (the same for every chromosome of a genome)."""
    sigma, mu = _numbers(f["sigma"]), _numbers(f["mu"])
    nu = mu * (1 - mu) / sigma ** 2 - 1
    return mu.shape[0], bool(f["is_kappa_fixed"]), mu * nu, (1 - mu) * nu


def _prepare(f, K: int, fixed: bool, seed: int, kappa, omega, p, positions, tot, meth):
    """One task's initial theta and the checks of its inputs, as `main` and
    `estimate_genome` both make them (p None: the default p)."""
    dim_theta = K * K if fixed else K * (K + 1)  # get_known_parameters (model_functions.R:48-54)
    if f["estimate_parameters"]:  # sampleFromParameterPriorCpp: theta ~ N(0, I) (singleGroup.h:480-483)
        theta_init = np.random.default_rng(seed).standard_normal(dim_theta)
    else:
        theta_init = theta_from_model(p if p is not None else default_p(K), omega, None if fixed else kappa)
    if tot.shape != meth.shape or tot.shape[0] != positions.shape[0]:
        raise ValueError(f"inconsistent inputs: positions {positions.shape}, totals {tot.shape}, "
                         f"methylated {meth.shape}")
    if np.any(meth > tot) or np.any(tot < 0) or np.any(tot != np.rint(tot)) or np.any(tot > 65535):
        raise ValueError("read counts must be integers with 0 <= methylated <= total <= 65535")
    return theta_init


def _write_outputs(f, paths, K: int, fixed: bool, kappa, positions, probs, theta) -> None:
    """One task's output files, for `main` and `estimate_genome` alike (paths:
    the file of each of the single command's output flags)."""
    if f["estimate_regime_probabilities"]:
        write_regimes(paths["regime_probabilities_csv_file"], positions, probs)
    if f["estimate_parameters"]:
        T = positions.shape[0]
        every = int(f["n_steps_without_parameter_update"])
        write_theta_trace(paths["theta_trace_csv_file"], theta, T, every)
        last = theta[(T - 1) // every]
        p_hat, omega_hat, kappa_hat = model_from_theta(last, K)
        write_csv(paths["p_csv_file"], [f"regime_{r + 1}" for r in range(K)],
                  [[_shortest(v) for v in p_hat[:, c]] for c in range(K)])
        write_vector(paths["omega_csv_file"], "omega", omega_hat)
        # the final estimate when kappa is estimated, else the given kappa (:363-369)
        write_vector(paths["kappa_csv_file"], "kappa", kappa if fixed else kappa_hat)
        write_vector(paths["theta_file"], "data", last, exp17=True)


# `hygeia estimate_genome`: the flags of estimate_parameters_and_regimes with
# the per-file ones replaced
_PER_FILE = ("p_input_csv_file", "kappa_input_csv_file", "omega_input_csv_file", "n_methylated_reads_csv_file",
             "genomic_positions_csv_file", "n_total_reads_csv_file", "regime_probabilities_csv_file",
             "theta_trace_csv_file", "omega_csv_file", "kappa_csv_file", "p_csv_file", "theta_file")
GENOME_FLAGS = [x for x in FLAGS if x[0] not in _PER_FILE and x[0] != "rng_seed"] + [
    ("rng_seed", "str", "-73"),
    ("data_dir", "str", None),
    ("group", "str", "control"),
    ("chroms", "str", "all"),
    ("output_dir", "str", None),
    ("parameters_dir", "str", None),
]


class GenomeError(GenomeInputError):
    """An input of `hygeia estimate_genome` that cannot be used (names the chromosome)."""


def _genome_inputs(group: str):
    return ("positions", f"n_total_reads_{group}", f"n_methylated_reads_{group}")


def genome_chroms(data_dir: str, group: str):
    """--chroms all: the chromosomes with their three files, numbered ones
    first in numeric order, then the rest by name (as cli.genome_chroms)."""
    import re

    found = []
    for name in (os.listdir(data_dir) if os.path.isdir(data_dir) else []):
        m = re.fullmatch(r"positions_(.+)\.txt\.gz", name)
        if m and all(os.path.exists(os.path.join(data_dir, f"{n}_{m.group(1)}.txt.gz"))
                     for n in _genome_inputs(group)):
            found.append(m.group(1))
    return sorted(found, key=lambda c: (0, int(c), "") if c.isdigit() else (1, 0, c))


def genome_output_paths(output_dir: str, chrom: str) -> Dict[str, str]:
    """The per-chromosome output names of 2_estimate_parameters_and_regimes.nf
    (what `hygeia infer --single_group_dir` reads), by the single command's flag."""
    j = lambda stem: os.path.join(output_dir, f"{stem}_{chrom}.csv.gz")  # noqa: E731
    return {"regime_probabilities_csv_file": j("regimes"), "theta_trace_csv_file": j("theta_trace"),
            "p_csv_file": j("p"), "kappa_csv_file": j("kappa"), "omega_csv_file": j("omega"),
            "theta_file": j("theta")}


def estimate_genome(argv: Sequence[str]) -> int:
    """`hygeia estimate_parameters_and_regimes` over chromosomes: every
    chromosome's chain in ONE launch (`run_engine_many`), each under its own
    model (its own theta_0 ~ N(0, I) from its seed with --estimate_parameters;
    its own p / kappa / omega from --parameters_dir without). Per chromosome the
    files are those of the single command run alone with that chromosome's
    files, parameters and seed. Every chromosome's files are read and checked
    before anything is written."""
    f = parse_flags(argv, GENOME_FLAGS)
    for name in ("data_dir", "output_dir"):
        if not f[name]:
            raise FlagError(f"--{name} is required")
    data_dir, out_dir, par_dir, group = str(f["data_dir"]), str(f["output_dir"]), f["parameters_dir"], str(f["group"])
    chroms = (genome_chroms(data_dir, group) if str(f["chroms"]) == "all"
              else [x for x in str(f["chroms"]).split(",") if x != ""])
    if len(set(chroms)) != len(chroms):
        raise GenomeError("--chroms names a chromosome twice")
    if not chroms:
        raise GenomeError(f"no chromosome to run: --chroms is empty, or no chromosome has its three files in {data_dir}")
    # one seed per chromosome (the seed of every draw of its task, :208-210)
    if f["randomise_rng_seed"]:
        seeds = [int.from_bytes(os.urandom(8), "little") for _ in chroms]
    else:
        try:
            given = [parse_int(x) for x in str(f["rng_seed"]).split(",") if x.strip() != ""]
        except ValueError:
            raise FlagError(f"invalid value for --rng_seed: {f['rng_seed']!r}")
        if len(given) == 1:
            given = given * len(chroms)
        if len(given) != len(chroms):
            raise GenomeError(f"--rng_seed has {len(given)} values for {len(chroms)} chromosomes "
                              f"({','.join(chroms)}): give one, or one per chromosome")
        seeds = [g & (2 ** 64 - 1) for g in given]
    u = int(f["u"])
    K, fixed, alpha, beta = _known_parameters(f)
    use_par = bool(par_dir) and not f["estimate_parameters"]
    tasks, meta, width = [], [], None
    for chrom, seed in zip(chroms, seeds):
        try:
            src = lambda n: os.path.join(data_dir, f"{n}_{chrom}.txt.gz")  # noqa: E731
            par = lambda n: os.path.join(str(par_dir), f"{n}_{chrom}.csv.gz")  # noqa: E731
            kappa = read_csv_matrix(par("kappa"))[:, 0] if use_par else _numbers(f["kappa"])
            omega = read_csv_matrix(par("omega"))[:, 0] if use_par else _numbers(f["omega"])
            p = read_csv_matrix(par("p")) if use_par else None
            names = _genome_inputs(group)
            positions = read_csv_matrix(src(names[0]))[:, 0]
            tot, meth = read_csv_matrix(src(names[1])), read_csv_matrix(src(names[2]))
            if kappa.shape[0] != K or omega.shape[0] != K or (p is not None and p.shape != (K, K)):
                raise ValueError(f"kappa, omega and p have {kappa.shape[0]}, {omega.shape[0]} and "
                                 f"{'x'.join(map(str, p.shape)) if p is not None else 'default'} entries, "
                                 f"the model has {K} regimes")
            theta_init = _prepare(f, K, fixed, seed, kappa, omega, p, positions, tot, meth)
            if tot.shape[0] < 1:
                raise ValueError("no sites")
            if width not in (None, tot.shape[1]):
                raise ValueError(f"{tot.shape[1]} samples, other chromosomes have {width}")
            width = tot.shape[1]
        except (OSError, EOFError, ValueError, IndexError) as e:  # what the readers raise on a missing or malformed file
            raise GenomeError(f"chromosome {chrom}: {type(e).__name__}: {e}") from e
        tasks.append({"meth": meth, "tot": tot, "theta_init": theta_init, "kappa": kappa, "seed": seed, "chain_id": 0})
        meta.append((chrom, kappa, positions))

    from . import _lib
    from .cli import _use_task_device

    L = _lib.load(import_torch=False)
    _use_task_device(L)
    results = run_engine_many(L, K, u, alpha, beta, f["epsilon"], f["n_particles"], tasks,
                              bool(f["estimate_parameters"]), f, is_kappa_fixed=fixed)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "rng_seeds.csv"), "w") as fh:
        fh.write("chrom,rng_seed\n" + "".join(f"{c},{s}\n" for c, s in zip(chroms, seeds)))
    for (chrom, kappa, positions), (probs, theta) in zip(meta, results):
        _write_outputs(f, genome_output_paths(out_dir, chrom), K, fixed, kappa, positions, probs, theta)
    return 0


# `hygeia sg_log_z`: the inputs of estimate_genome and a grid
SG_LOG_Z_FLAGS = [x for x in FLAGS if x[0] in ("mu", "sigma", "kappa", "omega", "is_kappa_fixed", "n_particles",
                                               "epsilon")] + [
    ("u", "str", "2"),
    ("seeds", "str", "-73"),
    ("data_dir", "str", None),
    ("group", "str", "control"),
    ("chroms", "str", "all"),
    ("output_dir", "str", None),
    ("parameters_dir", "str", "default"),
    ("trace", "flag", False),
]


def _int_list(f, name: str):
    try:
        vals = [parse_int(x) for x in str(f[name]).split(",") if x.strip() != ""]
    except ValueError:
        raise FlagError(f"invalid value for --{name}: {f[name]!r}")
    if not vals or len(set(vals)) != len(vals):
        raise FlagError(f"--{name} needs distinct integers, got {f[name]!r}")
    return vals


def sg_log_z(argv: Sequence[str]) -> int:
    """log Z of the single-group model over a grid: for every chromosome, every
    parameter set of --parameters_dir (directories holding p_ / kappa_ /
    omega_{chrom}.csv.gz as `estimate_genome` writes them; `default`: the flags'
    --kappa / --omega and the default p), every --u and every replicate seed of
    --seeds, the SMC estimate of log p(y) from forward-only launches
    (`filter_many`), one launch per --u value. The chains run with chain id 0,
    as `estimate_genome`'s: with a chromosome's seed from rng_seeds.csv a row is
    the log Z of that command's chain. Writes sg_log_z.tsv (a row per chromosome,
    parameter set, u and seed), sg_log_z_summary.tsv (per parameter set and u the
    sum over chromosomes of the log of the seeds' mean Z) and, with --trace, the
    filter trace of every row as sg_filter_{chrom}_{i}_{u}_{seed}.npz (i: the
    index of the parameter set). --epsilon is accepted and ignored (nothing is
    smoothed). Every file is read and checked before anything is written."""
    from .evidence import _write_tsv, log_mean_exp

    f = parse_flags(argv, SG_LOG_Z_FLAGS)
    for name in ("data_dir", "output_dir"):
        if not f[name]:
            raise FlagError(f"--{name} is required")
    data_dir, out_dir, group = str(f["data_dir"]), str(f["output_dir"]), str(f["group"])
    par_dirs = [x for x in str(f["parameters_dir"]).split(",") if x != ""]
    if not par_dirs or len(set(par_dirs)) != len(par_dirs):
        raise FlagError(f"--parameters_dir needs distinct directories (or `default`), got {f['parameters_dir']!r}")
    us, seeds = _int_list(f, "u"), _int_list(f, "seeds")
    if any(v < 1 for v in us):
        raise FlagError("--u needs positive integers")
    chroms = (genome_chroms(data_dir, group) if str(f["chroms"]) == "all"
              else [x for x in str(f["chroms"]).split(",") if x != ""])
    if len(set(chroms)) != len(chroms):
        raise GenomeError("--chroms names a chromosome twice")
    if not chroms:
        raise GenomeError(f"no chromosome to run: --chroms is empty, or no chromosome has its three files in {data_dir}")
    K, fixed, alpha, beta = _known_parameters(f)
    ff = dict(f, estimate_parameters=False)
    data, thetas, width = {}, {}, None  # chrom -> counts; (chrom, i) -> (theta, kappa)
    for chrom in chroms:
        try:
            src = lambda n: os.path.join(data_dir, f"{n}_{chrom}.txt.gz")  # noqa: E731
            names = _genome_inputs(group)
            positions = read_csv_matrix(src(names[0]))[:, 0]
            tot, meth = read_csv_matrix(src(names[1])), read_csv_matrix(src(names[2]))
            for i, d in enumerate(par_dirs):
                use_par = d != "default"
                par = lambda n: os.path.join(d, f"{n}_{chrom}.csv.gz")  # noqa: E731
                kappa = read_csv_matrix(par("kappa"))[:, 0] if use_par else _numbers(f["kappa"])
                omega = read_csv_matrix(par("omega"))[:, 0] if use_par else _numbers(f["omega"])
                p = read_csv_matrix(par("p")) if use_par else None
                if kappa.shape[0] != K or omega.shape[0] != K or (p is not None and p.shape != (K, K)):
                    raise ValueError(f"parameter set {d}: kappa, omega and p have {kappa.shape[0]}, {omega.shape[0]} "
                                     f"and {'x'.join(map(str, p.shape)) if p is not None else 'default'} entries, "
                                     f"the model has {K} regimes")
                thetas[(chrom, i)] = (_prepare(ff, K, fixed, 0, kappa, omega, p, positions, tot, meth), kappa)
            if tot.shape[0] < 1:
                raise ValueError("no sites")
            if width not in (None, tot.shape[1]):
                raise ValueError(f"{tot.shape[1]} samples, other chromosomes have {width}")
            width = tot.shape[1]
        except (OSError, EOFError, ValueError, IndexError) as e:
            raise GenomeError(f"chromosome {chrom}: {type(e).__name__}: {e}") from e
        data[chrom] = (np.ascontiguousarray(meth, dtype=np.uint16), np.ascontiguousarray(tot, dtype=np.uint16))

    from . import _lib
    from .cli import _use_task_device

    L = _lib.load(import_torch=False)
    _use_task_device(L)
    rows, traces = [], []
    for u in us:  # one launch per u: the models of a launch share it
        keys = [(chrom, i, seed) for chrom in chroms for i in range(len(par_dirs)) for seed in seeds]
        tasks = [{"meth": data[c][0], "tot": data[c][1], "theta_init": thetas[(c, i)][0], "kappa": thetas[(c, i)][1],
                  "seed": s & (2 ** 64 - 1), "chain_id": 0} for c, i, s in keys]
        res = filter_many(L, K, u, alpha, beta, f["n_particles"], tasks, trace=bool(f["trace"]), is_kappa_fixed=fixed)
        for (c, i, s), r in zip(keys, res):
            rows.append((c, par_dirs[i], u, s, data[c][1].shape[0], r["log_z"],
                         _lib.ERROR_NAMES.get(r["status"], r["status"])))
            if f["trace"]:
                traces.append((f"sg_filter_{c}_{i}_{u}_{s}.npz", r))
    os.makedirs(out_dir, exist_ok=True)
    _write_tsv(os.path.join(out_dir, "sg_log_z.tsv"),
               ("chrom", "parameters", "u", "seed", "n_sites", "log_z", "status"), rows)
    summary = []
    for d in par_dirs:
        for u in us:
            per = [log_mean_exp(np.array([r[5] for r in rows if r[0] == c and r[1] == d and r[2] == u]))
                   for c in chroms]
            summary.append((d, u, float(sum(per)), len(chroms), len(seeds)))
    _write_tsv(os.path.join(out_dir, "sg_log_z_summary.tsv"), ("parameters", "u", "log_z", "n_chroms", "n_seeds"),
               summary)
    for name, r in traces:
        np.savez(os.path.join(out_dir, name), log_z_t=r["log_z_t"], regime_probs=r["regime_probs"],
                 cp_probs=r["cp_probs"])
    return 0


# `hygeia sg_sample_genome`: sg_log_z's inputs without the grid and the trace
SG_SAMPLE_FLAGS = [x for x in SG_LOG_Z_FLAGS if x[0] not in ("trace", "u")] + [
    ("u", "int", 2),
    ("n_trajectories", "int", 25),
    ("history_gib", "double", 16.0),
    ("aggregate_dir", "str", None),
]


def history_bytes(n_sites: int, n_particles: int) -> int:
    """The history of one chain: log-weights f64 and states u32 per particle slot, the set's size i32 per site."""
    return (12 * int(n_particles) + 4) * int(n_sites)


def history_groups(lengths, n_seeds: int, n_particles: int, budget_bytes: float, names=None):
    """The launches of `sg_sample_genome`: the chromosomes (indices into
    `lengths`) longest first, each with all its seeds, packed first-fit into as
    few launches as fit the budget. A chromosome (`names[i]`, else its index)
    whose history alone exceeds the budget is a GenomeError naming both numbers."""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    groups, room = [], []
    for i in order:
        need = n_seeds * history_bytes(lengths[i], n_particles)
        if need > budget_bytes:
            raise GenomeError(f"chromosome {names[i] if names else i}: its history needs {need} bytes "
                              f"({n_seeds} seeds x {lengths[i]} sites x {12 * n_particles + 4} bytes), "
                              f"--history_gib allows {int(budget_bytes)} bytes")
        for g in range(len(groups)):
            if need <= room[g]:
                groups[g].append(i)
                room[g] -= need
                break
        else:
            groups.append([i])
            room.append(budget_bytes - need)
    return groups


def write_aggregate_matrices(out_dir: str, chrom: str, positions, regimes, durations) -> None:
    """The five per-chromosome matrices of `hygeia aggregate` (dmp.py's writer:
    a tab-separated frame indexed by pos, one column per trajectory) from a
    single group's draws: the group stands as control and as case, and every
    merge state is 1."""
    import pandas as pd

    pos = pd.Series(np.asarray(positions).astype(np.int32), name="pos")
    reg = pd.DataFrame(np.asarray(regimes)).astype(np.int8).set_index(pos)
    dur = pd.DataFrame(np.asarray(durations)).astype(np.int16).set_index(pos)
    merge = pd.DataFrame(np.ones(reg.shape, np.int8)).set_index(pos)
    for d, stem in ((reg, "control_regimes"), (reg, "case_regimes"), (dur, "control_durations"),
                    (dur, "case_durations"), (merge, "merge_states")):
        d.to_csv(os.path.join(out_dir, f"{stem}_chrom_{chrom}.csv.gz"), sep="\t", compression="gzip")


def sg_sample_genome(argv: Sequence[str]) -> int:
    """Joint segmentations of every chromosome by backward simulation
    (`sample_many`): for every chromosome and every replicate seed of --seeds,
    --n_trajectories draws of the whole path (d_t, r_t) under the parameters of
    --parameters_dir (`default`: the flags' --kappa / --omega and the default
    p). The chromosomes run in as few launches as fit --history_gib of particle
    history (12 n_particles + 4 bytes per site and seed), longest first. Writes
    sg_paths_{chrom}.npz (`positions`, `regimes` int8 [T][P], `durations` int16
    [T][P] modulo 2^16, P = seeds x n_trajectories, trajectory p = seed index x
    n_trajectories + b), sg_sample.tsv (chrom, seed, n_sites, log_z, status)
    and, with --aggregate_dir, the matrices `hygeia get_change_points` reads
    (`write_aggregate_matrices`). Every file is read and checked before
    anything is written."""
    from .evidence import _write_tsv

    f = parse_flags(argv, SG_SAMPLE_FLAGS)
    for name in ("data_dir", "output_dir"):
        if not f[name]:
            raise FlagError(f"--{name} is required")
    data_dir, out_dir, group, d = str(f["data_dir"]), str(f["output_dir"]), str(f["group"]), str(f["parameters_dir"])
    if d == "" or "," in d:
        raise FlagError(f"--parameters_dir needs one directory (or `default`), got {f['parameters_dir']!r}")
    seeds, u, B = _int_list(f, "seeds"), int(f["u"]), int(f["n_trajectories"])
    if u < 1:
        raise FlagError("--u needs a positive integer")
    if not 1 <= B <= 1024:
        raise FlagError(f"--n_trajectories must be in [1, 1024], got {B}")
    if not float(f["history_gib"]) > 0:
        raise FlagError(f"--history_gib must be positive, got {f['history_gib']!r}")
    chroms = (genome_chroms(data_dir, group) if str(f["chroms"]) == "all"
              else [x for x in str(f["chroms"]).split(",") if x != ""])
    if len(set(chroms)) != len(chroms):
        raise GenomeError("--chroms names a chromosome twice")
    if not chroms:
        raise GenomeError(f"no chromosome to run: --chroms is empty, or no chromosome has its three files in {data_dir}")
    K, fixed, alpha, beta = _known_parameters(f)
    ff = dict(f, estimate_parameters=False)
    use_par = d != "default"
    data, width = [], None  # per chromosome: positions, meth, tot, theta, kappa
    for chrom in chroms:
        try:
            src = lambda n: os.path.join(data_dir, f"{n}_{chrom}.txt.gz")  # noqa: E731
            par = lambda n: os.path.join(d, f"{n}_{chrom}.csv.gz")  # noqa: E731
            names = _genome_inputs(group)
            positions = read_csv_matrix(src(names[0]))[:, 0]
            tot, meth = read_csv_matrix(src(names[1])), read_csv_matrix(src(names[2]))
            kappa = read_csv_matrix(par("kappa"))[:, 0] if use_par else _numbers(f["kappa"])
            omega = read_csv_matrix(par("omega"))[:, 0] if use_par else _numbers(f["omega"])
            p = read_csv_matrix(par("p")) if use_par else None
            if kappa.shape[0] != K or omega.shape[0] != K or (p is not None and p.shape != (K, K)):
                raise ValueError(f"kappa, omega and p have {kappa.shape[0]}, {omega.shape[0]} and "
                                 f"{'x'.join(map(str, p.shape)) if p is not None else 'default'} entries, "
                                 f"the model has {K} regimes")
            theta = _prepare(ff, K, fixed, 0, kappa, omega, p, positions, tot, meth)
            if tot.shape[0] < 1:
                raise ValueError("no sites")
            if width not in (None, tot.shape[1]):
                raise ValueError(f"{tot.shape[1]} samples, other chromosomes have {width}")
            width = tot.shape[1]
        except (OSError, EOFError, ValueError, IndexError) as e:
            raise GenomeError(f"chromosome {chrom}: {type(e).__name__}: {e}") from e
        data.append((positions, np.ascontiguousarray(meth, dtype=np.uint16),
                     np.ascontiguousarray(tot, dtype=np.uint16), theta, kappa))
    lengths = [x[2].shape[0] for x in data]
    groups = history_groups(lengths, len(seeds), int(f["n_particles"]), float(f["history_gib"]) * 2 ** 30, chroms)

    from . import _lib
    from .cli import _use_task_device

    L = _lib.load(import_torch=False)
    _use_task_device(L)
    results = {}
    for g in groups:  # one launch pair per group
        keys = [(i, s) for i in g for s in seeds]
        tasks = [{"meth": data[i][1], "tot": data[i][2], "theta_init": data[i][3], "kappa": data[i][4],
                  "seed": s & (2 ** 64 - 1), "chain_id": 0} for i, s in keys]
        for k, r in zip(keys, sample_many(L, K, u, alpha, beta, f["n_particles"], tasks, B, is_kappa_fixed=fixed)):
            results[k] = r
    os.makedirs(out_dir, exist_ok=True)
    if f["aggregate_dir"]:
        os.makedirs(str(f["aggregate_dir"]), exist_ok=True)
    rows = []
    for i, chrom in enumerate(chroms):
        paths = np.concatenate([results[(i, s)]["paths"] for s in seeds], axis=1)  # [T][seeds x B][2]
        regimes, durations = paths[:, :, 1].astype(np.int8), np.ascontiguousarray(paths[:, :, 0])
        np.savez(os.path.join(out_dir, f"sg_paths_{chrom}.npz"), positions=data[i][0], regimes=regimes,
                 durations=durations)
        if f["aggregate_dir"]:
            write_aggregate_matrices(str(f["aggregate_dir"]), chrom, data[i][0], regimes, durations)
        for s in seeds:
            r = results[(i, s)]
            rows.append((chrom, s, lengths[i], r["log_z"], _lib.ERROR_NAMES.get(r["status"], r["status"])))
    _write_tsv(os.path.join(out_dir, "sg_sample.tsv"), ("chrom", "seed", "n_sites", "log_z", "status"), rows)
    return 0


def main(argv: Sequence[str]) -> int:
    f = parse_flags(argv)
    # the seed of every draw: --rng_seed when --randomise_rng_seed FALSE (:208-210)
    seed = int(f["rng_seed"]) & (2 ** 64 - 1) if not f["randomise_rng_seed"] else \
        int.from_bytes(os.urandom(8), "little")
    u = int(f["u"])
    kappa = (read_csv_matrix(f["kappa_input_csv_file"])[:, 0] if f["kappa_input_csv_file"]
             else _numbers(f["kappa"]))
    omega = (read_csv_matrix(f["omega_input_csv_file"])[:, 0] if f["omega_input_csv_file"]
             else _numbers(f["omega"]))
    K, fixed, alpha, beta = _known_parameters(f)
    p = read_csv_matrix(f["p_input_csv_file"]) if f["p_input_csv_file"] else None
    for path in (f["n_methylated_reads_csv_file"], f["genomic_positions_csv_file"], f["n_total_reads_csv_file"],
                 f["regime_probabilities_csv_file"], f["theta_trace_csv_file"], f["p_csv_file"],
                 f["omega_csv_file"], f["kappa_csv_file"], f["theta_file"]):  # create_dirs_for_file (:250-262)
        if isinstance(path, str) and os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
    positions = read_csv_matrix(f["genomic_positions_csv_file"])[:, 0]
    tot = read_csv_matrix(f["n_total_reads_csv_file"])
    meth = read_csv_matrix(f["n_methylated_reads_csv_file"])
    theta_init = _prepare(f, K, fixed, seed, kappa, omega, p, positions, tot, meth)

    from . import _lib
    from .cli import _use_task_device

    L = _lib.load(import_torch=False)
    _use_task_device(L)
    probs, theta = run_engine(L, K, u, alpha, beta, kappa, theta_init, f["epsilon"], f["n_particles"], meth, tot,
                              seed, 0, bool(f["estimate_parameters"]), f, is_kappa_fixed=fixed)
    _write_outputs(f, f, K, fixed, kappa, positions, probs, theta)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
