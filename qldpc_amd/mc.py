"""Monte-Carlo logical-error-rate driver: the outer loop of ``paperResults_GPU.py`` (:61-160),
sharded over the GPUs of one node.

One process per GPU (``torch.distributed``, backend ``nccl`` = RCCL over xGMI).  Trials are
independent, so each rank runs the contiguous slice ``[rank*T/R, (rank+1)*T/R)`` of the global
trial index range of every sweep point through ``qbp_mc_run_device`` (sampling, decoding and
classification all on the device; include/qbp.h) and the only communication is ONE all-reduce
(sum, int64) of the ``[points, 12]`` counter table at the end of the sweep.  Errors are drawn
from a counter-based generator keyed by the GLOBAL trial index, so the counters are identical
for every world size -- that is the multi-GPU correctness test (tests/test_mc_distributed.py).

    python -m qldpc_amd.mc --code 288 --p 0.06 0.05 0.04 --trials 1000000
    python -m torch.distributed.run --nproc-per-node 8 -m qldpc_amd.mc --code 288 ...
    python -m qldpc_amd.mc --dem circuit.dem --trials 1000000 --osd      (detector error model: run_dem)
    python -m qldpc_amd.mc --dem circuit.dem --shots dets.b8 --obs obs.b8 --osd --predictions-out pred.npy
                                     (decode RECORDED shots to observable predictions: run_shots)
    python -m qldpc_amd.mc --circuit 72 6 --p 0.001 0.002 --shots 1000000 --osd [--basis X]
                                     (circuit-level noise: the memory experiment sampled and decoded on the device: run_circuit)
    python -m qldpc_amd.mc --circuit 72 6 --fault-weights 2 4 6 8 --prior-p 0.001 --trials 1000000 --osd --ler-at 1e-4 1e-3
                                     (exactly w firing fault sites, and the circuit-level LER at any p from their failure
                                      fractions: run_circuit_weights, ler_from_weights)
    python -m qldpc_amd.mc --code 288 --p 0.01 --osd --budgets 10 20 30 40 50 60 70 80 90
                                     (a ladder of iteration limits in one pass: run_budgets, BP_per_Iteration.py)
    python -m qldpc_amd.mc --code 288 --p 0.01 --osd --budgets 10 20 30 --llr-hist 128 -30 30 --out ladder.json
                                     (and the posterior-LLR histograms per limit: run_llr_hist; table in ladder.npz)
    python -m qldpc_amd.mc --code 144 --p 0.05 --osd --spectrum out.npz
                                     (residual-weight spectra and the iteration histogram per point: run_spectrum)
    python -m qldpc_amd.mc --code 144 --depolarizing 0.01 0.02 --trials 100000 --osd
                                     (Pauli noise on both sectors, two-stage X/Z-correlated decoding: run_depolarizing)
    python -m qldpc_amd.mc --code 144 --weights 4 6 8 10 12 --prior-p 0.01 --trials 1000000 --osd --ler-at 0.001 0.003 0.01
                                     (errors of fixed weight, and the LER at any p from their failure fractions:
                                      run_weights, ler_from_weights)
    python -m qldpc_amd.mc --code 72 --enumerate 1 2 3 --prior-p 0.01 --osd --failures out.npz --failures-what either
                                     (EVERY error of these weights: exact failure fractions and the failing patterns,
                                      run_enumerate, enumerate.failing_patterns; with --weights one LER from both)
"""
from __future__ import annotations

import argparse
import collections
import json
import math
import os
import time

import numpy as np

from . import _lib, codes

NUM_COUNTERS = _lib.NUM_COUNTERS
_VARIANTS = {"sum-product": _lib.SUM_PRODUCT, "damped": _lib.DAMPED_SP, "min-sum": _lib.MIN_SUM}   # (--variant)


def shard_range(trials: int, rank: int, world: int):
    """Contiguous slice of [0, trials) owned by `rank`; slices tile the range exactly."""
    return rank * trials // world, (rank + 1) * trials // world


def prior_of(p: float, n: int) -> np.ndarray:
    return np.full(n, np.log((1 - p) / p))          # paperResults_GPU.py:79


def summarize(counters: np.ndarray) -> dict:
    """Counter row -> the per-point quantities the reference stores / prints."""
    c = {k: int(v) for k, v in zip(_lib.COUNTER_NAMES, counters)}
    t = max(c["trials"], 1)
    c["ler"] = c["logical_error"] / t                                   # :146 (BP+OSD when osd)
    # BP-only convention of notebooks/data/BP.npz: a non-converged trial counts as a failure
    c["ler_bp_only"] = (c["logical_error"] - c["logical_error_not_converged"]
                        + c["not_converged"]) / t
    c["mean_iterations"] = c["sum_iterations"] / t + 1.0
    return c


def osd_run_flags(osd, osd_method="cs", osd_order=0, osd_large=False) -> int:
    """Flags of the OSD pass of a sweep: 0 without OSD, FLAG_OSD0 for OSD-0 (order 0), else order-w OSD
    (``_lib.osd_flags``; ``osd_large``: FLAG_OSD_LARGE, order w also on matrices beyond the one-wavefront OSD
    kernel).  ValueError for an order without ``osd``, ``osd_large`` with order 0 or a method / order out of range."""
    fl = _lib.osd_flags(osd_method, osd_order, osd_large)   # (validates method, order and osd_large)
    if not osd:
        if int(osd_order) != 0:
            raise ValueError(f"an OSD order ({osd_order}) needs osd=True")
        return 0
    return fl


def relay_run_flags(flags, relay) -> int:
    """``flags`` of a sweep with ``relay`` (None, a ``relay.RelayConfig`` or its dict form): | FLAG_RELAY, the trials BP
    leaves unconverged go to Relay-BP.  ValueError together with OSD: one second stage per run."""
    if relay is None:
        return flags
    if flags & (_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | _lib.FLAG_OSD_LARGE):
        raise ValueError("relay= and osd=True exclude each other: one second stage per run")
    return flags | _lib.FLAG_RELAY


def gd_run_flags(flags, gd) -> int:
    """``flags`` of a sweep with ``gd`` (None, a ``gd.GDConfig`` or its dict form): | FLAG_GD, the trials BP leaves
    unconverged go to BP guided decimation.  ValueError together with OSD or Relay-BP: one second stage per run."""
    if gd is None:
        return flags
    if flags & (_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | _lib.FLAG_OSD_LARGE | _lib.FLAG_RELAY):
        raise ValueError("gd= excludes osd=True and relay=: one second stage per run")
    from . import gd as gd_mod
    gd_mod.as_config(gd)                # (a bad configuration raises here, before any GPU work)
    return flags | _lib.FLAG_GD


def lsd_run_flags(flags, lsd, lsd_large=False) -> int:
    """``flags`` of a sweep with ``lsd`` (None, or the bits_per_step of localized statistics decoding): | FLAG_LSD, the
    trials BP leaves unconverged go to LSD.  ValueError together with OSD, Relay-BP or BPGD: one second stage per run;
    for an ``lsd_large`` that ``Decoder.lsd_configure(large=)`` does not accept, or one without ``lsd``."""
    _lib.msg_mem_value("lsd", lsd_large)
    if lsd is None:
        if lsd_large:
            raise ValueError("lsd_large= needs lsd=")
        return flags
    if flags & (_lib.FLAG_OSD0 | _lib.FLAG_OSD_CS | _lib.FLAG_OSD_E | _lib.FLAG_OSD_LARGE | _lib.FLAG_RELAY | _lib.FLAG_GD):
        raise ValueError("lsd= excludes osd=True, relay= and gd=: one second stage per run")
    from . import lsd as lsd_mod
    lsd_mod.check_bits_per_step(lsd)    # (a bad value raises here, before any GPU work)
    return flags | _lib.FLAG_LSD


def _configure_lsd(dec, lsd, lsd_large=False):
    if lsd is not None:
        dec.lsd_configure(lsd, lsd_large)


def _configure_gd(dec, gd):
    if gd is not None:
        from . import gd as gd_mod
        dec.gd_configure(gd_mod.as_config(gd))


def _configure_relay(dec, relay):
    if relay is not None:
        from . import relay as relay_mod
        dec.relay_configure(relay_mod.as_config(relay, dec.n))


def layered_run_flags(flags, layered, variant) -> int:
    """``flags`` of a sweep with ``layered`` (False / None, True = the default order, "large" = the default order, also
    on matrices beyond the LDS, or a permutation of the checks): | FLAG_LAYERED, BP runs the layered schedule.
    ValueError with the damped variant, which has no layered form, and with any other string."""
    if layered is None or layered is False:
        return flags
    if isinstance(layered, str) and layered != "large":
        raise ValueError(f"layered must be False, True, 'large' or an order of the checks, got {layered!r}")
    if int(variant) == _lib.DAMPED_SP:
        raise ValueError("layered=True needs variant sum-product or min-sum: there is no damped layered schedule")
    return flags | _lib.FLAG_LAYERED


def _configure_layered(dec, layered):
    """True: the default order, OPT_LAYERED_MEM 0 (LDS only, as ever); "large": the default order, OPT_LAYERED_MEM 2
    (the messages in a global workspace where the LDS does not hold them); an array: that order, the option as it is."""
    if layered is None or layered is False:
        return
    if isinstance(layered, str):
        dec.layered_configure(None, large=True)
    elif layered is True:
        dec.layered_configure(None, large=False)
    else:
        dec.layered_configure(layered)


def quant_run_flags(flags, quant, layered, variant) -> int:
    """``flags`` of a sweep with ``quant`` (None, a ``quant.QuantConfig`` or its dict form): | FLAG_QUANT, the first stage
    is fixed-point min-sum.  ValueError for a bad configuration, together with ``layered``, or with a variant other than
    min-sum."""
    if quant is None:
        return flags
    from . import quant as quant_mod
    quant_mod.as_config(quant)          # (a bad value raises here, before any GPU work)
    if layered is not None and layered is not False:
        raise ValueError("quant= excludes layered=: one first stage per run")
    if int(variant) != _lib.MIN_SUM:
        raise ValueError("quant= needs variant min-sum: fixed-point BP is min-sum")
    return flags | _lib.FLAG_QUANT


def _configure_quant(dec, quant):
    if quant is not None:
        from . import quant as quant_mod
        dec.quant_configure(quant_mod.as_config(quant))


def _stages(variant, *, osd=False, osd_method="cs", osd_order=0, osd_large=False, relay=None, layered=False, gd=None,
            lsd=None, lsd_large=False, quant=None):
    """The decoder stages of a run, stated once: ``(flags, configure)`` -- the flags word of its calls, and
    ``configure(dec)``, which sets a decoder up for them.  Every ValueError of a bad value or combination is raised
    here, before any GPU work.  A driver that takes fewer stages passes fewer keywords."""
    flags = relay_run_flags(osd_run_flags(osd, osd_method, osd_order, osd_large), relay)
    flags = layered_run_flags(lsd_run_flags(gd_run_flags(flags, gd), lsd, lsd_large), layered, variant)
    flags = quant_run_flags(flags, quant, layered, variant)

    def configure(dec):
        _configure_relay(dec, relay)
        _configure_gd(dec, gd)
        _configure_lsd(dec, lsd, lsd_large)
        _configure_layered(dec, layered)
        _configure_quant(dec, quant)
    return flags, configure


def _on_device(shape, priors, ranges, step, launch, world, device, reduce=True):
    """One rank's share of a run on the device, then the ONE all-reduce of its int64 table of ``shape`` (zeroed here;
    returned as a numpy array; ``reduce=False``: this rank's table as it is).  A point per entry of ``priors``, each
    owning an equal share of the table; ``ranges``: this rank's ``(begin, end)`` -- a tuple, the same for every point
    -- or a list of them, one per point.  ``launch(i, d_prior, a, b, d_out, stream)`` enqueues trials [a, b) of point
    i, which add to the share at address ``d_out``; ``step`` trials at the most per launch
    (``Decoder.mc_step``)."""
    import torch
    dev = torch.device("cuda", device)
    d_table = torch.zeros(shape, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_priors = [torch.from_numpy(np.ascontiguousarray(prior, np.float64)).to(dev) for prior in priors]
    shares = d_table.view(len(priors), d_table.numel() // max(len(priors), 1))
    if isinstance(ranges, tuple):
        ranges = [ranges] * len(priors)
    for i, (d_prior, d_out, (begin, end)) in enumerate(zip(d_priors, shares, ranges)):
        for a in range(begin, end, step):
            launch(i, d_prior.data_ptr(), a, min(a + step, end), d_out.data_ptr(), stream)
    if world > 1 and reduce:
        import torch.distributed as dist
        dist.all_reduce(d_table)                     # the one RCCL collective of the run
    torch.cuda.synchronize(dev)
    return d_table.cpu().numpy()


def _mc_code(code_name):
    """``codes.load_code`` for the Monte-Carlo entries, which classify logical errors against ``distance // 2``: a
    code without a distance (``codes.register`` of a new code) is refused here, before any GPU work."""
    code = codes.load_code(code_name)
    if code.distance is None:
        raise ValueError(f"code {code.name!r} has no distance: run qldpc_amd.distance.estimate(code) first (it sets "
                         f"code.distance to the upper bound it finds), or give one to codes.from_matrices")
    return code


def run_sweep(code_name, ps, trials, *, draws=1, seed=0, max_iter=50, variant=_lib.SUM_PRODUCT,
              alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0,
              world=1, device=0, runner=None, all_reduce=None, relay=None, layered=False, gd=None, lsd=None,
              lsd_large=False, quant=None):
    """Returns the GLOBAL counter table int64[len(ps), 12] (after the reduce).

    ``quant``: a ``quant.QuantConfig`` or its dict form -- the first stage is fixed-point min-sum (FLAG_QUANT; variant
    min-sum only, not together with ``layered``); ``alpha``, ``damping`` and ``clip_llr`` are not read.  Every second
    stage acts on what it leaves unconverged.

    ``lsd``: the bits_per_step (>= 0) of localized statistics decoding on the trials BP does not converge on (FLAG_LSD;
    not together with ``osd``, ``relay`` or ``gd``); ``lsd_large`` (False, True, "force"; ``lsd.py``) allows matrices
    whose rows pass 160 KiB of LDS or number more than 2048 (OPT_LSD_MEM).

    ``gd``: a ``gd.GDConfig`` or its dict form -- BP guided decimation on the trials BP does not converge on (FLAG_GD;
    not together with ``osd`` or ``relay``); its ``large`` (False, True, "auto") allows matrices whose record state
    passes 160 KiB of LDS (OPT_GD_MEM).

    ``layered``: True -- BP runs the layered (check-serial) schedule in its default order (FLAG_LAYERED); an array -- in
    that order of the checks; "large" -- the default order, with the messages in a global workspace on matrices whose
    record state passes 160 KiB of LDS (OPT_LAYERED_MEM 2; True refuses those).  OSD and Relay act on what it leaves
    unconverged.

    ``relay``: a ``relay.RelayConfig`` or its dict form -- Relay-BP instead of OSD on the trials BP does not converge
    on (FLAG_RELAY; not together with ``osd``).

    ``osd``: OSD on the trials BP does not converge on -- OSD-0 with ``osd_order`` 0, else order-w OSD by
    ``osd_method`` ("cs" or "e"; include/qbp.h).
    `runner(code, p, begin, end) -> int64[12]` and `all_reduce(int64 array) -> int64 array`
    are injection points for the CPU tests; by default the HIP library and torch.distributed."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               relay=relay, layered=layered, gd=gd, lsd=lsd, lsd_large=lsd_large, quant=quant)
    code = _mc_code(code_name)
    begin, end = shard_range(trials, rank, world)
    if runner is None:
        from . import bp
        dec = bp.decoder_for(code.Hx, device=device)
        configure(dec)

        def launch(i, d_prior, a, b, d_out, stream):
            dec.mc_run_device(code.Lx, code.distance, ps[i], d_prior, a, b, d_out, draws=draws, seed=seed,
                              max_iter=max_iter, variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr,
                              flags=flags, stream=stream)
        return _on_device((len(ps), NUM_COUNTERS), [prior_of(p, code.n) for p in ps], (begin, end),
                          dec.mc_step(flags, end - begin), launch, world, device)
    table = np.zeros((len(ps), NUM_COUNTERS), np.int64)
    for i, p in enumerate(ps):
        table[i] = runner(code, p, begin, end)
    return all_reduce(table) if all_reduce is not None else table


def pauli_rates(p, bias=(1, 1, 1)):
    """(px, py, pz) of Pauli noise of total strength ``p`` split in the proportions ``bias`` = (X, Y, Z); (1, 1, 1)
    is depolarizing noise."""
    b = [float(x) for x in bias]
    if len(b) != 3 or min(b) < 0.0 or sum(b) <= 0.0:
        raise ValueError(f"bias must be three weights >= 0 with a positive sum, got {bias!r}")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"p must be in [0, 1], got {p!r}")
    return tuple(float(p) * x / sum(b) for x in b)


def run_depolarizing(code_name, ps, trials, *, osd=False, osd_method="cs", osd_order=0, bias=(1, 1, 1), correlated=True,
                     seed=0, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, rank=0,
                     world=1, device=0):
    """Logical error rates of a CSS code under Pauli noise, both sectors decoded (qbp_css_mc_run): returns the GLOBAL
    table int64[len(ps), 3, 12] -- per point the counter rows of sector A (Hx, Lx: Z and Y errors), of sector B (Hz, Lz:
    X and Y errors) and of the trial as a whole (row 2: [1] is a logical error in either sector).

    ``correlated``: the second stage's prior is conditioned on the first stage's correction (``css.pauli_priors``);
    False passes the marginal prior of sector B for both cases, which decodes the sectors independently on the same
    errors -- the baseline.  ``bias``: the proportions of X, Y and Z in ``p``.  Trials are sharded over ranks as in
    ``run_sweep`` and the tables summed with one all-reduce; errors are keyed by the global trial index, so the table
    does not depend on the world size."""
    from . import bp, css
    flags = osd_run_flags(osd, osd_method, osd_order)
    code = _mc_code(code_name)
    rates = [pauli_rates(p, bias) for p in ps]         # (before any GPU work)
    priors = []
    for px, py, pz in rates:
        pa, b0, b1 = css.pauli_priors(px, py, pz, code.n)
        if not correlated:
            b0 = b1 = css.marginal_prior_b(px, py, pz, code.n)
        priors.append((pa, b0, b1))
    dec = _lib.CssDecoder(bp.decoder_for(code.Hx, device=device), bp.decoder_for(code.Hz, device=device))
    begin, end = shard_range(trials, rank, world)
    table = np.zeros((len(ps), 3, NUM_COUNTERS), np.int64)
    for i, ((px, py, pz), (pa, b0, b1)) in enumerate(zip(rates, priors)):
        dec.mc_run(code.Lx, code.Lz, code.distance, px, py, pz, pa, b0, b1, begin, end, seed=seed, max_iter=max_iter,
                   variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr, flags=flags, counters=table[i])
    if world > 1:
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(table)
        if dist.get_backend() == "nccl":
            t = t.to(torch.device("cuda", device))
        dist.all_reduce(t)
        table = t.cpu().numpy()
    return table


def dem_prior(probs) -> np.ndarray:
    """Default prior of a detector error model: log((1 - p) / p) with p clipped to [1e-15, 1 - 1e-15]
    (studies/studyComplete.py:85-86)."""
    p = np.clip(np.asarray(probs, np.float64), 1e-15, 1 - 1e-15)
    return np.log((1 - p) / p)


def _dem_args(H, L, probs, prior):
    """The arguments of a run on a matrix H [m, n], as ``(L uint8[k, n], probs float64[n], prior float64[n], n)``: at
    most 64 observables; ``probs`` None for a run without them; ``prior`` None: ``dem_prior(probs)``.  ValueError
    for any other shape."""
    L = np.ascontiguousarray(L, np.uint8)
    n = H.shape[1]
    if L.ndim != 2 or L.shape[1] != n:
        raise ValueError(f"L must have shape (k, {n}), got {L.shape}")
    if L.shape[0] > 64:
        raise ValueError(f"at most 64 observables (got {L.shape[0]})")
    if probs is not None:
        probs = np.ascontiguousarray(probs, np.float64)
        if probs.shape != (n,):
            raise ValueError(f"probs must have shape ({n},), got {probs.shape}")
    prior = dem_prior(probs) if prior is None and probs is not None else np.ascontiguousarray(prior, np.float64)
    if prior.shape != (n,):
        raise ValueError(f"prior must have shape ({n},), got {prior.shape}")
    return L, probs, prior, n


# What a run decodes, resolved once from a code name or from a matrix: H [m, n], L [k, n], the distance of the
# miscorrected / incorrectable split, n, and per point the sampler's argument (``probs``: an error rate, or a
# probability per column; None where the entry samples by other means) and the decoder's LLRs (``priors``).
_Model = collections.namedtuple("_Model", "H L distance n probs priors")


def _code_model(code, ps):
    """The model of a built-in or registered code (``_mc_code``): its X sector, a point per error rate of ``ps``."""
    return _Model(code.Hx, code.Lx, code.distance, code.n, [float(p) for p in ps], [prior_of(p, code.n) for p in ps])


def _matrix_model(H, L, probs, prior, distance):
    """The one-point model of a matrix with observables (``_dem_args`` checks and completes it)."""
    L, probs, prior, n = _dem_args(H, L, probs, prior)
    return _Model(H, L, distance, n, [probs], [prior])


def _bind(runner, *lead):
    """An injected ``runner`` with its leading arguments (the code and rate, or the matrix and its tables) bound: what
    the shared body of a pair of drivers calls.  None stays None: the HIP library runs."""
    return None if runner is None else lambda *args: runner(*lead, *args)


def run_dem(H, L, probs, trials, *, prior=None, distance=0, draws=1, seed=0, max_iter=50,
            variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs",
            osd_order=0, osd_large=False, rank=0, world=1, device=0, runner=None, all_reduce=None, relay=None,
            layered=False, gd=None, window=None, check_round=None, lsd=None, lsd_large=False, quant=None):
    """Monte-Carlo on a detector error model (``dem.parse_dem`` / ``dem.phenomenological``): column v of H [m, n]
    fails with probability probs[v] (qbp_mc_run_probs), BP [+ OSD] decodes the syndrome with ``prior`` (default
    ``dem_prior(probs)``), and a trial is a logical error when ``L @ (error ^ correction) != 0`` -- the
    ``L_matrix @ prediction != actual_observables`` of studies/studyComplete.py.  Returns the GLOBAL counters
    int64[12] (after one all-reduce), sharded over ranks like ``run_sweep``.

    ``distance``: the "BPs_miscorrected" / "incorrectable" split compares the error weight with distance // 2;
    the default 0 counts every logical error as "incorrectable" (a DEM does not say its distance).
    ``runner(H, L, probs, prior, begin, end) -> int64[12]`` and ``all_reduce`` are injection points for the CPU
    tests (with ``window`` the runner is also passed ``window=(W, F), check_round=``); by default the HIP library and
    torch.distributed.  ``relay``, ``layered``, ``gd``, ``lsd``, ``lsd_large``, ``quant``: as in ``run_sweep``.

    ``window``: ``(W, F)`` -- the sliding-window decoder (qbp_window_mc_run_probs; ``window.py``) with the round of
    every check in ``check_round``; "not_converged" then counts the trials with a window BP did not converge on.  Not
    together with ``relay``, ``layered``, ``gd`` or ``lsd``.  Sharded and reduced exactly like the plain path."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               relay=relay, layered=layered, gd=gd, lsd=lsd, lsd_large=lsd_large, quant=quant)
    L, probs, prior, n = _dem_args(H, L, probs, prior)
    begin, end = shard_range(int(trials), rank, world)
    extra = {}                          # (what a window adds to the runner's arguments)
    if window is not None:
        if relay is not None or gd is not None or (layered is not None and layered is not False):
            raise ValueError("window= runs flooding BP [+ OSD] inside a window: not with relay, layered or gd")
        if lsd is not None:
            raise ValueError("window= runs flooding BP [+ OSD] inside a window: not with lsd")
        if quant is not None:
            raise ValueError("window= runs flooding BP [+ OSD] inside a window: not with quant")
        if check_round is None:
            raise ValueError("window= needs check_round, the round of every check of H")
        W, F = (int(x) for x in window)
        extra = dict(window=(W, F), check_round=check_round)
    if runner is None:
        if window is None:
            from . import bp
            dec = bp.decoder_for(H, device=device)
            configure(dec)
            step = dec.mc_step(flags, end - begin)
        else:
            from . import window as window_mod
            dec = window_mod.decoder_for(H, check_round, W, F, device=device)
            step = max(end - begin, 1)          # (one call: the window entry splits a long range into chunks itself)

        def launch(i, d_prior, a, b, d_out, stream):
            dec.mc_run_probs_device(L, distance, probs, d_prior, a, b, d_out, draws=draws, seed=seed, max_iter=max_iter,
                                    variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr, flags=flags,
                                    stream=stream)
        return _on_device((NUM_COUNTERS,), [prior], (begin, end), step, launch, world, device)
    cnt = np.asarray(runner(H, L, probs, prior, begin, end, **extra), np.int64)
    return all_reduce(cnt) if all_reduce is not None else cnt


def run_shots(H, L, detections, observables=None, *, prior, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0,
              damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, flags=0, rank=0, world=1, device=0,
              runner=None, all_reduce=None):
    """Decode RECORDED shots of a detector error model to observable predictions (qbp_decode_shots): the loop of
    studies/studyComplete.py:91-109 on data that was sampled elsewhere (stim's circuit sampler, an experiment).

    ``detections``: the detection events, bit-packed uint8 [T, ceil(m / 8)] (``shots.pack_bits`` /
    ``shots.read_shots``) or a 0/1 array [T, m]; where ceil(m / 8) == m (m = 1) a uint8 array is taken as packed.
    ``observables``: None, the recorded flips as uint64 masks [T] (bit l = observable l) or a 0/1 array [T, k].
    ``prior``: the decoder's LLRs [n] (``dem_prior(probs)`` for a model's own rates).  ``flags``: further
    decoder flags (column-sum order, FLAG_FORCE_FULL), or-ed with the OSD flags of ``osd`` / ``osd_method`` /
    ``osd_order``.

    Returns ``(counters int64[12], predictions uint64[T_local], converged bool[T_local])``.  The shot range is split
    over ranks with ``shard_range``; the counters are GLOBAL (one all-reduce: [0] shots, [1] prediction != recorded,
    [6] not converged, [7] iterations, [8] the [1] among [6], [10] OSD outputs that miss the syndrome), while
    predictions and converged cover THIS RANK'S slice ``shard_range(T, rank, world)`` only, in shot order.
    ``runner(H, L, det_bits, masks, prior, begin, end) -> (int64[12], uint64[end - begin], bool[end - begin])`` and
    ``all_reduce`` are injection points for the CPU tests; by default the HIP library and torch.distributed."""
    from . import shots as shots_mod
    flags = int(flags) | osd_run_flags(osd, osd_method, osd_order, osd_large)     # (before any GPU work)
    m, n = H.shape
    rb = (m + 7) // 8
    L = np.ascontiguousarray(L, np.uint8)
    if L.ndim != 2 or L.shape[1] != n:
        raise ValueError(f"L must have shape (k, {n}), got {L.shape}")
    if not 1 <= L.shape[0] <= 64:
        raise ValueError(f"1 to 64 observables (got {L.shape[0]})")
    det = np.asarray(detections)
    if det.ndim != 2:
        raise ValueError(f"detections must be [T, {rb}] packed bytes or a [T, {m}] 0/1 array, got shape {det.shape}")
    if det.dtype == np.uint8 and det.shape[1] == rb:
        det = np.ascontiguousarray(det)
    elif det.shape[1] == m:
        det = shots_mod.pack_bits(det)            # (C-contiguous whatever the order of the input)
    else:
        raise ValueError(f"detections must be [T, {rb}] packed bytes or a [T, {m}] 0/1 array, got {det.dtype} "
                         f"{det.shape}")
    T = det.shape[0]
    masks = None
    det = np.ascontiguousarray(det)
    if observables is not None:
        obs = np.asarray(observables)
        masks = np.ascontiguousarray(shots_mod.masks_of(obs) if obs.ndim == 2 else np.asarray(obs, np.uint64))
        if obs.ndim == 2 and obs.shape[1] != L.shape[0]:
            raise ValueError(f"observables must have {L.shape[0]} columns, got {obs.shape[1]}")
        if masks.shape != (T,):
            raise ValueError(f"observables must cover the {T} shots, got shape {obs.shape}")
    prior = np.ascontiguousarray(prior, np.float64)
    if prior.shape != (n,):
        raise ValueError(f"prior must have shape ({n},), got {prior.shape}")
    if np.isnan(prior).any():
        raise ValueError("prior holds NaN")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be >= 1, got {max_iter}")
    begin, end = shard_range(T, rank, world)
    if runner is None:
        import torch

        from . import bp
        dec = bp.decoder_for(H, device=device)
        dev = torch.device("cuda", device)
        d_det = torch.from_numpy(det[begin:end]).to(dev)
        d_act = torch.from_numpy(masks[begin:end].view(np.int64)).to(dev) if masks is not None else None
        d_pred = torch.zeros(end - begin, dtype=torch.int64, device=dev)
        d_conv = torch.zeros(end - begin, dtype=torch.uint8, device=dev)

        def launch(i, d_prior, a, b, d_out, stream):
            o = a - begin                                     # (the per-shot buffers hold this rank's slice only)
            dec.decode_shots_device(L, d_det.data_ptr() + o * rb, d_act.data_ptr() + 8 * o if d_act is not None else 0,
                                    b - a, d_prior, d_pred.data_ptr() + 8 * o, d_conv.data_ptr() + o, d_out,
                                    max_iter=max_iter, variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr,
                                    flags=flags, stream=stream)
        cnt = _on_device((NUM_COUNTERS,), [prior], (begin, end), dec.mc_step(flags, end - begin), launch, world, device)
        return cnt, d_pred.cpu().numpy().view(np.uint64), d_conv.cpu().numpy().astype(bool)
    cnt, pred, conv = runner(H, L, det, masks, prior, begin, end)
    cnt = np.asarray(cnt, np.int64)
    cnt = all_reduce(cnt) if all_reduce is not None else cnt
    return cnt, np.asarray(pred, np.uint64), np.asarray(conv, bool)


def run_circuit(code, rounds, ps, shots, *, basis="Z", idle=True, detectors="basis", rates=None, seed=0, max_iter=50,
                variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0,
                osd_large=False, flags=0, chunk=None, rank=0, world=1, device=0, reduce=True):
    """Logical error rate of a CSS code under circuit-level noise (studies/studyComplete.py:72-109 without stim): the
    memory experiment ``circuit.memory_experiment(code, rounds, basis, idle, detectors)`` and its detector error model
    ``circuit.circuit_dem`` are built once; per point p the rates are ``{every class: p}`` (or ``rates[i]``, rates per
    class as ``circuit.rates_array`` takes them, one entry per point) and the prior is ``dem_prior(dem.probs(rates))``.
    Per chunk of shots qbp_frame_sample_device samples detection rows and observable masks on the device and
    qbp_decode_shots_device decodes them with the masks as the recorded observables: nothing returns to the host
    between chunks.  Returns the GLOBAL int64 [points, 12] counters of ``run_shots`` (LER = [1] / [0]); the shot range
    is split over ranks with ``shard_range`` and the counters do not depend on ``chunk``, rank or world.
    ``flags``: further decoder flags, or-ed with the OSD flags.  ``reduce=False``: this rank's counters, without the
    all-reduce (tests add the ranks up themselves)."""
    from . import bp, circuit as circuit_mod
    flags = int(flags) | osd_run_flags(osd, osd_method, osd_order, osd_large)     # (before any GPU work)
    ps = [float(p) for p in ps]
    if rates is not None and len(rates) != len(ps):
        raise ValueError(f"rates must have one entry per point ({len(ps)}), got {len(rates)}")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be >= 1, got {max_iter}")
    cir = circuit_mod.memory_experiment(code, rounds, basis=basis, idle=idle, detectors=detectors)
    point_rates = [circuit_mod.rates_array(p if rates is None else rates[i], cir.n_classes) for i, p in enumerate(ps)]
    import torch
    cdem = circuit_mod.circuit_dem(cir, device=device)
    sim = cir.simulator(device)
    dec = bp.decoder_for(cdem.H, device=device)
    rb = (cdem.H.shape[0] + 7) // 8
    step = min(dec.mc_step(flags, 1 << 20), 1 << 20)      # (a chunk's detection rows are a buffer: capped in any case)
    if chunk is not None:
        step = max(1, min(step, int(chunk)))
    begin, end = shard_range(int(shots), rank, world)
    dev = torch.device("cuda", device)
    d_det = torch.zeros(max(min(step, end - begin), 1) * max(rb, 1), dtype=torch.uint8, device=dev)
    d_obs = torch.zeros(max(min(step, end - begin), 1), dtype=torch.int64, device=dev)

    def launch(i, d_prior, a, b, d_out, stream):          # (sample a chunk into the two buffers, then decode it)
        sim.sample_device(point_rates[i], b - a, d_det.data_ptr(), d_obs.data_ptr(), seed=seed, shot_begin=a,
                          stream=stream)
        dec.decode_shots_device(cdem.L, d_det.data_ptr(), d_obs.data_ptr(), b - a, d_prior, 0, 0, d_out,
                                max_iter=max_iter, variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr,
                                flags=flags, stream=stream)
    return _on_device((len(ps), NUM_COUNTERS), [dem_prior(cdem.probs(r)) for r in point_rates], (begin, end), step,
                      launch, world, device, reduce=reduce)


def _budgets(model, run, trials, budgets, flags, *, rank, world, device, all_reduce, **decoder):
    """The body of ``run_budgets`` and ``run_dem_budgets``: this rank's slice of the ladder on the one point of
    ``model`` -- on the device with the one all-reduce of the [K, 12] table, or through ``run(budgets, begin, end)`` and
    ``all_reduce``.  ``decoder``: the keywords of ``Decoder.mc_run_budgets_device``."""
    begin, end = shard_range(int(trials), rank, world)
    if run is None:
        from . import bp
        dec = bp.decoder_for(model.H, device=device)

        def launch(i, d_prior, a, b, d_out, stream):
            dec.mc_run_budgets_device(model.L, model.distance, model.probs[0], d_prior, budgets, a, b, d_out, flags=flags,
                                      stream=stream, **decoder)
        return _on_device((len(budgets), NUM_COUNTERS), model.priors, (begin, end),
                          dec.mc_step(flags, end - begin, len(budgets)), launch, world, device)
    table = np.asarray(run(budgets, begin, end), np.int64).reshape(len(budgets), NUM_COUNTERS)
    return all_reduce(table) if all_reduce is not None else table


def run_budgets(code_name, p, trials, budgets, *, draws=1, seed=0, variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0,
                clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0, world=1, device=0, runner=None,
                all_reduce=None):
    """One error rate, a ladder of BP iteration limits, ONE pass over the trials (qbp_mc_run_budgets): returns the
    GLOBAL counter table int64[len(budgets), 12] whose row j is the row ``run_sweep(code_name, [p], trials,
    max_iter=budgets[j], ...)`` returns -- the sweep of BP_per_Iteration.py:40-81.  Sharded and reduced like
    ``run_sweep`` (one all-reduce of the table).  ValueError, before any GPU work, for budgets that are not 1 to
    ``_lib.MC_MAX_BUDGETS`` strictly ascending integers >= 1.
    ``runner(code, p, budgets, begin, end) -> int64[K, 12]`` and ``all_reduce`` are injection points for the CPU
    tests; by default the HIP library and torch.distributed."""
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)   # (before any GPU work)
    budgets = _lib.check_budgets(budgets)
    code = _mc_code(code_name)
    return _budgets(_code_model(code, [p]), _bind(runner, code, p), trials, budgets, flags, rank=rank, world=world,
                    device=device, all_reduce=all_reduce, draws=draws, seed=seed, variant=variant, alpha=alpha,
                    damping=damping, clip_llr=clip_llr)


def run_dem_budgets(H, L, probs, trials, budgets, *, prior=None, distance=0, draws=1, seed=0,
                    variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs",
                    osd_order=0, osd_large=False, rank=0, world=1, device=0, runner=None, all_reduce=None):
    """``run_dem`` over a ladder of BP iteration limits in one pass: GLOBAL int64[len(budgets), 12], row j = the
    counters of ``run_dem(..., max_iter=budgets[j])``.  Arguments as ``run_dem``, budgets as ``run_budgets``;
    ``runner(H, L, probs, prior, budgets, begin, end) -> int64[K, 12]``."""
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)
    budgets = _lib.check_budgets(budgets)
    model = _matrix_model(H, L, probs, prior, distance)
    return _budgets(model, _bind(runner, H, model.L, model.probs[0], model.priors[0]), trials, budgets, flags, rank=rank,
                    world=world, device=device, all_reduce=all_reduce, draws=draws, seed=seed, variant=variant,
                    alpha=alpha, damping=damping, clip_llr=clip_llr)


def _split_llr_hist(flat, K, bins):
    """[K * 12 + K * 4 * (bins + 3)] -> (counters [K, 12], hist [K, 4, bins + 3]): the layout the LLR-histogram runs
    reduce in one piece."""
    flat = np.asarray(flat, np.int64).ravel()
    a = K * NUM_COUNTERS
    return flat[:a].reshape(K, NUM_COUNTERS).copy(), flat[a:].reshape(K, _lib.LLR_HIST_ROWS, bins + 3).copy()


def _llr_hist(model, run, trials, budgets, bins, llr_range, flags, *, rank, world, device, all_reduce, **decoder):
    """The body of ``run_llr_hist`` and ``run_dem_llr_hist``: this rank's slice of the ladder with its LLR table on the
    one point of ``model`` -- counters and table side by side in one int64 row, reduced in one piece -- on the device,
    or through ``run(budgets, bins, llr_range, begin, end)`` and ``all_reduce``.  ``decoder``: the keywords of
    ``Decoder.mc_run_llr_hist_device``."""
    K = len(budgets)
    begin, end = shard_range(int(trials), rank, world)
    if run is None:
        from . import bp
        dec = bp.decoder_for(model.H, device=device)

        def launch(i, d_prior, a, b, d_out, stream):
            dec.mc_run_llr_hist_device(model.L, model.distance, model.probs[0], d_prior, budgets, bins, llr_range, a, b,
                                       d_out, d_out + 8 * K * NUM_COUNTERS, flags=flags, stream=stream, **decoder)
        width = K * NUM_COUNTERS + K * _lib.LLR_HIST_ROWS * (bins + 3)
        flat = _on_device((1, width), model.priors, (begin, end), dec.mc_step(flags, end - begin, K), launch, world,
                          device)
    else:
        flat = np.concatenate([np.asarray(a, np.int64).ravel()
                               for a in run(budgets, bins, llr_range, begin, end)])[None, :]
        flat = all_reduce(flat) if all_reduce is not None else flat
    return (*_split_llr_hist(flat, K, bins), _lib.llr_hist_edges(bins, *llr_range))


def run_llr_hist(code_name, p, trials, budgets, bins, llr_range, *, draws=1, seed=0, variant=_lib.SUM_PRODUCT, alpha=1.0,
                 damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0, world=1,
                 device=0, runner=None, all_reduce=None):
    """``run_budgets`` plus the distribution of BP's posterior LLRs per iteration limit (qbp_mc_run_llr_hist).  Returns
    GLOBAL ``(counters int64[K, 12], hist int64[K, 4, bins + 3], edges float64[bins + 1])``: the counters are
    ``run_budgets``' digit for digit; ``hist[j, 2 * (BP did not converge) + true bit, c]`` counts, over all trials and
    all n bits, the posterior values a decode with ``max_iter=budgets[j]`` returns, in column c -- 0 below
    ``llr_range[0]``, 1 .. bins the bins of ``np.histogram(x, bins, range=llr_range)`` (``edges``), bins + 1 above
    ``llr_range[1]``, bins + 2 NaN.  The lists of BP_per_Iteration.py:46-60 binned: ``llrs_per_iter[j]`` is
    ``hist[j].sum(0)``, ``llrs_per_iter_after_OSD[j]`` is ``hist[j, 2] + hist[j, 3]``.  Sharded like ``run_budgets``;
    counters and table are reduced in ONE all-reduce.  ValueError, before any GPU work, for what the library refuses
    (``_lib.check_budgets``, ``_lib.check_llr_hist``).
    ``runner(code, p, budgets, bins, llr_range, begin, end) -> (int64[K, 12], int64[K, 4, bins + 3])`` and
    ``all_reduce`` are injection points for the CPU tests; by default the HIP library and torch.distributed."""
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)   # (before any GPU work)
    budgets = _lib.check_budgets(budgets)
    bins, lo, hi = _lib.check_llr_hist(bins, *llr_range, len(budgets))
    code = _mc_code(code_name)
    return _llr_hist(_code_model(code, [p]), _bind(runner, code, p), trials, budgets, bins, (lo, hi), flags, rank=rank,
                     world=world, device=device, all_reduce=all_reduce, draws=draws, seed=seed, variant=variant,
                     alpha=alpha, damping=damping, clip_llr=clip_llr)


def run_dem_llr_hist(H, L, probs, trials, budgets, bins, llr_range, *, prior=None, distance=0, draws=1, seed=0,
                     variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs",
                     osd_order=0, osd_large=False, rank=0, world=1, device=0, runner=None, all_reduce=None):
    """``run_dem_budgets`` with the table of ``run_llr_hist``: GLOBAL ``(counters int64[K, 12], hist int64[K, 4, bins +
    3], edges)`` for a matrix with a probability per column.  Arguments as ``run_dem`` and ``run_llr_hist``;
    ``runner(H, L, probs, prior, budgets, bins, llr_range, begin, end) -> (int64[K, 12], int64[K, 4, bins + 3])``."""
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)
    budgets = _lib.check_budgets(budgets)
    bins, lo, hi = _lib.check_llr_hist(bins, *llr_range, len(budgets))
    model = _matrix_model(H, L, probs, prior, distance)
    return _llr_hist(model, _bind(runner, H, model.L, model.probs[0], model.priors[0]), trials, budgets, bins, (lo, hi),
                     flags, rank=rank, world=world, device=device, all_reduce=all_reduce, draws=draws, seed=seed,
                     variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr)


def bp_per_iteration(code_names, p, budgets, trials, osd=True, llr_bins=None, llr_range=None, **kwargs):
    """The result dictionary of BP_per_Iteration.py:85-88: per code name ``logicalErrors``, ``degeneracies`` and
    ``OSD_invocations`` (rates per trial, one entry per iteration limit) and ``iterations`` (the limits).  One
    ``run_budgets`` pass per code; ``kwargs`` go to it.

    With ``llr_bins`` and ``llr_range=(lo, hi)`` the pass is ``run_llr_hist`` and every entry gains the script's
    per-limit LLR lists (:46-60, :82-90, its violin plots) as histograms: ``llrs_per_iter_hist`` and
    ``llrs_per_iter_after_OSD_hist`` (the posteriors of the trials BP left unconverged), int64[K, llr_bins + 3] each
    with the columns of ``run_llr_hist``, and ``llr_edges``.  Without them the result is what it always was."""
    if (llr_bins is None) != (llr_range is None):
        raise ValueError("llr_bins and llr_range go together")
    results = {}
    for name in code_names:
        if llr_bins is None:
            table = run_budgets(name, p, trials, budgets, osd=osd, **kwargs)
        else:
            table, hist, edges = run_llr_hist(name, p, trials, budgets, llr_bins, llr_range, osd=osd, **kwargs)
        t = np.maximum(table[:, 0], 1).astype(np.float64)
        results[name] = {
            "logicalErrors": (table[:, 1] / t).tolist(),            # :76-79
            "degeneracies": (table[:, 5] / t).tolist(),             # :73-74, :80
            "OSD_invocations": (table[:, 6] / t).tolist(),          # :58-64, :81 (trials BP left unconverged)
            "iterations": [int(b) for b in budgets],
        }
        if llr_bins is not None:
            results[name].update(llrs_per_iter_hist=hist.sum(axis=1), llrs_per_iter_after_OSD_hist=hist[:, 2] + hist[:, 3],
                                 llr_edges=edges)
    return results


def llr_distributions(code_name, p, trials, max_iter, bins, llr_range, **kwargs):
    """The posterior-LLR distributions of rework/Alvarado.py:122, 159-162, split by the TRUE value of the bit:
    ``{"true_0": int64[bins + 3], "true_1": int64[bins + 3], "edges": float64[bins + 1]}`` over all bits of ``trials``
    decodes with ``max_iter`` (``run_llr_hist`` with one budget: rows 0 + 2 and 1 + 3; columns as there -- [1:bins + 1]
    are ``np.histogram``'s counts of the script's ``llr_data[...]["true_0"]`` / ``["true_1"]`` lists).  ``kwargs`` go
    to ``run_llr_hist``."""
    _, hist, edges = run_llr_hist(code_name, p, trials, [int(max_iter)], bins, llr_range, **kwargs)
    return {"true_0": hist[0, 0] + hist[0, 2], "true_1": hist[0, 1] + hist[0, 3], "edges": edges}


def _split_spectrum(flat, n, max_iter):
    """[points, 12 + 4 (n + 1) + max_iter + 1] -> (counters [points, 12], weights [points, 4, n + 1], iterations
    [points, max_iter + 1]): the layout the spectrum runs reduce in one piece."""
    flat = np.asarray(flat, np.int64)
    a, b = NUM_COUNTERS, NUM_COUNTERS + _lib.SPECTRUM_ROWS * (n + 1)
    return (flat[:, :a].copy(), flat[:, a:b].reshape(len(flat), _lib.SPECTRUM_ROWS, n + 1).copy(),
            flat[:, b:b + max_iter + 1].copy())


def _spectrum(model, run, trials, max_iter, flags, *, rank, world, device, all_reduce, **decoder):
    """The body of ``run_spectrum`` and ``run_dem_spectrum``: this rank's slice of every point of ``model`` --
    counters, weights and iterations of a point side by side in one int64 row, the table reduced in one piece -- on
    the device, or through ``run(i, begin, end)`` per point and ``all_reduce``.  ``decoder``: the keywords of
    ``Decoder.mc_run_spectrum_device``."""
    n, points = model.n, len(model.priors)
    begin, end = shard_range(int(trials), rank, world)
    if run is None:
        from . import bp
        dec = bp.decoder_for(model.H, device=device)

        def launch(i, d_prior, a, b, d_out, stream):
            dec.mc_run_spectrum_device(model.L, model.distance, model.probs[i], d_prior, a, b, d_out,
                                       d_out + 8 * NUM_COUNTERS, d_out + 8 * (NUM_COUNTERS + _lib.SPECTRUM_ROWS * (n + 1)),
                                       max_iter=max_iter, flags=flags, stream=stream, **decoder)
        width = NUM_COUNTERS + _lib.SPECTRUM_ROWS * (n + 1) + max_iter + 1
        flat = _on_device((points, width), model.priors, (begin, end), dec.mc_step(flags, end - begin), launch, world,
                          device)
    else:
        flat = np.stack([np.concatenate([np.asarray(a, np.int64).ravel() for a in run(i, begin, end)])
                         for i in range(points)]) if points else np.zeros((0, 0), np.int64)
        flat = all_reduce(flat) if all_reduce is not None else flat
    return _split_spectrum(flat, n, max_iter)


def _check_spectrum_max_iter(max_iter):
    if not 1 <= int(max_iter) <= _lib.MC_SPECTRUM_MAX_ITER:
        raise ValueError(f"a spectrum run takes max_iter in [1, {_lib.MC_SPECTRUM_MAX_ITER}], got {max_iter}")
    return int(max_iter)


def run_spectrum(code_name, ps, trials, *, draws=1, seed=0, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0,
                 damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0, world=1, device=0,
                 runner=None, all_reduce=None):
    """``run_sweep`` with a distribution per point (qbp_mc_run_spectrum).  Returns GLOBAL ``(counters int64[points,
    12], weights int64[points, 4, n + 1], iterations int64[points, max_iter + 1])``: the counters are ``run_sweep``'s
    digit for digit; ``weights[i, r, w]`` counts the trials of point i whose residual has weight w > 0 in list r of
    rework/main.py:65-112 (0 weights_found_BP, 1 weights_found_OSD, 2 weights_found_BP_error, 3
    weights_found_OSD_error; spectrum.py's list is rows 0 + 1); ``iterations[i, k]`` counts the trials whose syndrome
    was first satisfied in 0-based iteration k, ``iterations[i, max_iter]`` those BP did not converge on.  Sharded
    like ``run_sweep``; counters and tables are reduced in ONE all-reduce.
    ``runner(code, p, begin, end) -> (int64[12], int64[4, n + 1], int64[max_iter + 1])`` and ``all_reduce`` are
    injection points for the CPU tests; by default the HIP library and torch.distributed."""
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)   # (before any GPU work)
    max_iter = _check_spectrum_max_iter(max_iter)
    code = _mc_code(code_name)
    run = None if runner is None else lambda i, begin, end: runner(code, ps[i], begin, end)
    return _spectrum(_code_model(code, ps), run, trials, max_iter, flags, rank=rank, world=world, device=device,
                     all_reduce=all_reduce, draws=draws, seed=seed, variant=variant, alpha=alpha, damping=damping,
                     clip_llr=clip_llr)


def run_dem_spectrum(H, L, probs, trials, *, prior=None, distance=0, draws=1, seed=0, max_iter=50,
                     variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs",
                     osd_order=0, osd_large=False, rank=0, world=1, device=0, runner=None, all_reduce=None):
    """``run_dem`` with the two distributions of ``run_spectrum``: GLOBAL ``(counters int64[1, 12], weights int64[1,
    4, n + 1], iterations int64[1, max_iter + 1])`` -- one point, the model's own probabilities.  Arguments as
    ``run_dem``; ``runner(H, L, probs, prior, begin, end) -> (int64[12], int64[4, n + 1], int64[max_iter + 1])``."""
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)
    max_iter = _check_spectrum_max_iter(max_iter)
    model = _matrix_model(H, L, probs, prior, distance)
    run = None if runner is None else lambda i, begin, end: runner(H, model.L, model.probs[0], model.priors[0], begin, end)
    return _spectrum(model, run, trials, max_iter, flags, rank=rank, world=world, device=device, all_reduce=all_reduce,
                     draws=draws, seed=seed, variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr)


def check_weights(weights, n, what="n columns"):
    """The weights of a fixed-weight run as a list of ints in [0, n] (ValueError otherwise -- the library refuses the
    same values with QBP_E_INVALID); ``what``: what n counts, for the message."""
    w = np.asarray(weights)
    if w.ndim != 1 or w.dtype.kind not in "iu":
        raise ValueError(f"weights must be a list of integers, got {weights!r}")
    if np.any(w < 0) or np.any(w > n):
        raise ValueError(f"weights must lie in [0, {n}] ({what}), got {weights!r}")
    return [int(x) for x in w]


def _weights(model, run, weights, trials, flags, configure, *, rank, world, device, all_reduce,
             entry="mc_run_weight_device", top=None, reduce=True, **decoder):
    """The body of ``run_weights``, ``run_weights_matrix`` and ``run_circuit_weights``: this rank's slice of the trials
    of every weight, decoded with the one prior of ``model`` -- on the device with the one all-reduce of the
    [len(weights), 12] table, or through ``run(w, begin, end)`` per weight and ``all_reduce``.  ``entry``: the
    ``Decoder`` method that enqueues a range of one weight, ``decoder`` its keywords; ``top``: the largest weight it
    takes and what that counts, ``(number, words)`` -- default the n columns of the model."""
    weights = check_weights(weights, *((model.n,) if top is None else top))
    begin, end = shard_range(int(trials), rank, world)
    if run is None:
        from . import bp
        dec = bp.decoder_for(model.H, device=device)
        configure(dec)
        enqueue = getattr(dec, entry)

        def launch(i, d_prior, a, b, d_out, stream):
            enqueue(model.L, model.distance, weights[i], d_prior, a, b, d_out, flags=flags, stream=stream, **decoder)
        return _on_device((len(weights), NUM_COUNTERS), model.priors * len(weights), (begin, end),
                          dec.mc_step(flags, end - begin), launch, world, device, reduce=reduce)
    table = np.zeros((len(weights), NUM_COUNTERS), np.int64)
    for i, w in enumerate(weights):
        table[i] = run(w, begin, end)
    return all_reduce(table) if all_reduce is not None else table


def run_weights(code_name, weights, trials, *, prior_p, seed=0, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0,
                damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0, world=1,
                device=0, runner=None, all_reduce=None, relay=None, layered=False, gd=None, lsd=None,
                lsd_large=False, quant=None):
    """Monte-Carlo stratified by error weight (qbp_mc_run_weight): for every w of ``weights``, ``trials`` errors of
    exactly w ones, uniform among the C(n, w) patterns, decoded with the prior of error rate ``prior_p`` -- which fixes
    the decoder the failure fractions are measured for.  Returns the GLOBAL counter table int64[len(weights), 12];
    ``ler_from_weights`` turns it into the logical error rate at any p.  Shards, steps and reduces as ``run_sweep``
    does (trials of every weight are split over ranks; one all-reduce of the table).
    ``runner(code, w, begin, end) -> int64[12]`` and ``all_reduce`` are injection points for the CPU tests; by default
    the HIP library and torch.distributed.  ``relay``, ``layered``, ``gd``, ``lsd``, ``lsd_large``, ``quant``: as in
    ``run_sweep``."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               relay=relay, layered=layered, gd=gd, lsd=lsd, lsd_large=lsd_large, quant=quant)
    code = _mc_code(code_name)
    return _weights(_code_model(code, [prior_p]), _bind(runner, code), weights, trials, flags, configure, rank=rank,
                    world=world, device=device, all_reduce=all_reduce, seed=seed, max_iter=max_iter, variant=variant,
                    alpha=alpha, damping=damping, clip_llr=clip_llr)


def run_weights_matrix(H, L, weights, trials, *, prior, distance=0, seed=0, max_iter=50, variant=_lib.SUM_PRODUCT,
                       alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False,
                       rank=0, world=1, device=0, runner=None, all_reduce=None, lsd=None, lsd_large=False, quant=None):
    """``run_weights`` for any matrix H [m, n] with logical operators / observables L [k, n] (k <= 64) and the
    decoder's LLRs ``prior`` [n].  The weight classes are the strata of UNIFORM noise -- every column failing with the
    same p; under per-column probabilities the patterns of one weight are not equiprobable, and ``ler_from_weights``
    does not apply.  (The detector error model of a circuit is that case: ``run_circuit_weights`` stratifies it by the
    number of firing fault SITES instead, for which the formula holds.)  ``distance`` as in ``run_dem``.  ``runner(H, L, w, prior, begin, end) -> int64[12]``.  ``lsd``,
    ``lsd_large``, ``quant``: as in ``run_sweep``; of the stages of ``run_weights`` a matrix takes these and OSD."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               lsd=lsd, lsd_large=lsd_large, quant=quant)
    model = _matrix_model(H, L, None, prior, distance)
    run = None if runner is None else lambda w, begin, end: runner(H, model.L, w, model.priors[0], begin, end)
    return _weights(model, run, weights, trials, flags, configure, rank=rank, world=world, device=device,
                    all_reduce=all_reduce, seed=seed, max_iter=max_iter, variant=variant, alpha=alpha, damping=damping,
                    clip_llr=clip_llr)


def _circuit_fault_model(code, rounds, weights, prior_p, classes, basis, idle, detectors, device):
    """What a fixed-weight fault run of a memory experiment needs, built once: ``(circuit, CircuitDem, model, table,
    weights)`` -- the one-point ``_Model`` on the DEM's H and L with the prior ``dem_prior(cdem.probs(rates))``,
    ``rates`` being ``prior_p`` on the classes of ``classes`` (None: every class) and 0 elsewhere, ``table =
    (first_fault, K, N)`` of the active sites, and the weights as ``check_weights`` returns them.  ValueError, before
    any GPU work: ``prior_p`` outside (0, 1), an unknown class, no active site, or a weight outside
    [0, min(N, FAULT_WEIGHT_MAX)]."""
    from . import circuit as circuit_mod
    prior_p = float(prior_p)
    if not 0.0 < prior_p < 1.0:
        raise ValueError(f"prior_p = {prior_p} out of (0, 1)")
    cir = circuit_mod.memory_experiment(code, rounds, basis=basis, idle=idle, detectors=detectors)
    table = circuit_mod.fault_sites(cir, classes)
    N = table[2]
    if N == 0:
        raise ValueError(f"no fault site in the rate classes {classes!r}")
    weights = check_weights(weights, min(N, _lib.FAULT_WEIGHT_MAX),
                            f"min of N = {N} active fault sites and {_lib.FAULT_WEIGHT_MAX}")
    active = range(cir.n_classes) if classes is None else sorted(circuit_mod._class_set(classes))
    rates = circuit_mod.rates_array({int(c): prior_p for c in active}, cir.n_classes)
    cdem = circuit_mod.circuit_dem(cir, device=device)
    model = _matrix_model(cdem.H, cdem.L, cdem.probs(rates), None, 0)
    return cir, cdem, model, table, weights


def run_circuit_weights(code, rounds, weights, trials, *, prior_p, classes=None, basis="Z", idle=True, detectors="basis",
                        seed=0, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False,
                        osd_method="cs", osd_order=0, osd_large=False, lsd=None, lsd_large=False, quant=None, rank=0,
                        world=1, device=0, reduce=True):
    """Circuit-level Monte-Carlo stratified by the number of firing fault SITES (qbp_mc_run_fault_weight): the memory
    experiment ``circuit.memory_experiment(code, rounds, basis, idle, detectors)`` and its detector error model are
    built once, as in ``run_circuit``; for every w of ``weights``, ``trials`` fault sets of exactly w distinct active
    sites, uniform among the C(N, w) site sets, each site with one of its K codes, uniform, are mapped to error rows
    over the DEM's columns on the device and decoded by the pipeline of ``run_weights_matrix``.  Active sites: those
    whose rate class is in ``classes`` (None: all; ``circuit.fault_sites``).  The prior is
    ``dem_prior(cdem.probs(rates))`` with ``prior_p`` on the active classes and 0 elsewhere; it fixes the decoder the
    failure fractions are measured for.

    Returns ``(table int64[len(weights), 12], N)``.  When every active site fires with the same rate p, independently,
    ``ler_from_weights(table, weights, N, ps)`` is the logical error rate at every p -- ``Circuit.sample``'s model with
    one rate; unequal rates between active classes are out of scope (the site set given w is then not uniform).
    Weights lie in [0, min(N, 256)].  Shards, steps and reduces as ``run_weights`` does; ``reduce=False``: this rank's
    table.  ``lsd``, ``lsd_large``, ``quant``: as in ``run_weights_matrix``."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               lsd=lsd, lsd_large=lsd_large, quant=quant)
    _, cdem, model, (first, K, N), weights = _circuit_fault_model(code, rounds, weights, prior_p, classes, basis, idle,
                                                                  detectors, device)

    def configure_faults(dec):
        configure(dec)
        dec.fault_table_set(first, K, cdem.fault_column)
    table = _weights(model, None, weights, trials, flags, configure_faults, rank=rank, world=world, device=device,
                     all_reduce=None, entry="mc_run_fault_weight_device", reduce=reduce,
                     top=(min(N, _lib.FAULT_WEIGHT_MAX), f"min of N = {N} active fault sites and {_lib.FAULT_WEIGHT_MAX}"),
                     seed=seed, max_iter=max_iter, variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr)
    return table, N


def circuit_failing_faults(code, rounds, weight, trials, *, prior_p, classes=None, basis="Z", idle=True,
                           detectors="basis", what="logical", cap=1 << 20, seed=0, max_iter=50,
                           variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0, clip_llr=20.0, osd=False, osd_method="cs",
                           osd_order=0, osd_large=False, device=0):
    """WHICH fault sets of ``run_circuit_weights`` the decoder fails on (qbp_fault_weight_failures): trials
    [0, ``trials``) of weight ``weight`` are decoded as ``run_shots`` decodes their detection events (flooding BP
    [+ OSD]) and those of kind ``what`` ("logical", "unconverged" or "either") are captured, at most ``cap`` of them.
    Returns a dict: ``trials`` int64 [F] (ascending when found <= cap), ``kinds`` uint8 [F] (bit 0 a logical failure,
    bit 1 BP did not converge), ``found``, ``counters`` int64 [12], ``N``, and ``faults`` int64 [F, weight], the fault
    numbers of every captured trial (``circuit.fault_sets``), with ``sites`` and ``codes`` of the same shape: the site in
    the circuit's site numbering and the code 1 .. K of every fault."""
    from . import bp, circuit as circuit_mod
    kinds_of = {"logical": 1, "unconverged": 2, "either": 3}
    if what not in kinds_of:
        raise ValueError(f"what must be one of {sorted(kinds_of)}, got {what!r}")
    flags = osd_run_flags(osd, osd_method, osd_order, osd_large)
    if int(cap) < 0 or int(trials) < 0:
        raise ValueError("cap and trials must be >= 0")
    cir, cdem, model, (first, K, N), (weight,) = _circuit_fault_model(code, rounds, [weight], prior_p, classes, basis,
                                                                      idle, detectors, device)
    dec =bp.decoder_for(model.H, device=device)
    dec.fault_table_set(first, K, cdem.fault_column)
    hit, kinds, found, counters = dec.fault_weight_failures(
        model.L, weight, model.priors[0], 0, int(trials), seed=seed, what=kinds_of[what], cap=cap, max_iter=max_iter,
        variant=variant, alpha=alpha, damping=damping, clip_llr=clip_llr, flags=flags)
    faults = circuit_mod.fault_sets(cir, weight, seed, hit, classes)
    base = cir.sites()[5]
    sites = np.searchsorted(base, faults, side="right") - 1
    return dict(trials=hit, kinds=kinds, found=found, counters=counters, N=N, faults=faults, sites=sites,
                codes=faults - base[sites] + 1)


def _enumerate(model, run, weights, flags, configure, *, rank, world, device, all_reduce, **decoder):
    """The body of ``run_enumerate`` and ``run_enumerate_matrix``: ``_weights`` with a range per weight -- this rank's
    share ``shard_range(C(n, w), rank, world)`` of the ranks of every class.  ``decoder``: the keywords of
    ``Decoder.mc_run_enum_device``."""
    from . import enumerate as enum_mod
    weights = check_weights(weights, model.n)
    counts = [enum_mod.count(model.n, w) for w in weights]
    ranges = [shard_range(c, rank, world) for c in counts]
    if run is None:
        from . import bp
        dec = bp.decoder_for(model.H, device=device)
        configure(dec)

        def launch(i, d_prior, a, b, d_out, stream):
            dec.mc_run_enum_device(model.L, model.distance, weights[i], d_prior, a, b, d_out, flags=flags, stream=stream,
                                   **decoder)
        return _on_device((len(weights), NUM_COUNTERS), model.priors * len(weights), ranges,
                          dec.mc_step(flags, max(counts, default=1)), launch, world, device)
    table = np.zeros((len(weights), NUM_COUNTERS), np.int64)
    for i, (w, (begin, end)) in enumerate(zip(weights, ranges)):
        table[i] = run(w, begin, end)
    return all_reduce(table) if all_reduce is not None else table


def run_enumerate(code_name, weights, *, prior_p, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0, damping=1.0,
                  clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0, world=1, device=0,
                  runner=None, all_reduce=None, relay=None, layered=False, gd=None, lsd=None, lsd_large=False, quant=None):
    """``run_weights`` on EVERY pattern of each weight instead of sampled ones (qbp_mc_run_enum): the C(n, w) patterns
    of every w of ``weights`` in the order of ``enumerate.unrank``, each class sharded over ranks by
    ``shard_range(C(n, w), rank, world)``; one all-reduce.  Row i of the GLOBAL table has [0] == C(n, weights[i]) exactly
    and [1] / [0] is the exact f_w (``ler_from_weights(..., exact_weights=weights)``).  A class of more than 2^62
    patterns is a ValueError.  ``runner(code, w, begin, end) -> int64[12]`` gets a rank range; the other keywords are
    ``run_weights``'s."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               relay=relay, layered=layered, gd=gd, lsd=lsd, lsd_large=lsd_large, quant=quant)
    code = _mc_code(code_name)
    return _enumerate(_code_model(code, [prior_p]), _bind(runner, code), weights, flags, configure, rank=rank, world=world,
                      device=device, all_reduce=all_reduce, max_iter=max_iter, variant=variant, alpha=alpha,
                      damping=damping, clip_llr=clip_llr)


def run_enumerate_matrix(H, L, weights, *, prior, distance=0, max_iter=50, variant=_lib.SUM_PRODUCT, alpha=1.0,
                         damping=1.0, clip_llr=20.0, osd=False, osd_method="cs", osd_order=0, osd_large=False, rank=0,
                         world=1, device=0, runner=None, all_reduce=None, lsd=None, lsd_large=False, quant=None):
    """``run_enumerate`` for any matrix, as ``run_weights_matrix`` is ``run_weights`` for any matrix.
    ``runner(H, L, w, prior, begin, end) -> int64[12]``."""
    flags, configure = _stages(variant, osd=osd, osd_method=osd_method, osd_order=osd_order, osd_large=osd_large,
                               lsd=lsd, lsd_large=lsd_large, quant=quant)
    model = _matrix_model(H, L, None, prior, distance)
    run = None if runner is None else lambda w, begin, end: runner(H, model.L, w, model.priors[0], begin, end)
    return _enumerate(model, run, weights, flags, configure, rank=rank, world=world, device=device,
                      all_reduce=all_reduce, max_iter=max_iter, variant=variant, alpha=alpha, damping=damping,
                      clip_llr=clip_llr)


def merge_weight_tables(enum_table, enum_weights, sampled_table, sampled_weights):
    """An enumerated table (``run_enumerate``) and a sampled one (``run_weights``) as one ``(table, weights)`` for
    ``ler_from_weights`` -- pass ``exact_weights=enum_weights`` there.  A weight present in both is a ValueError."""
    a, b = np.asarray(enum_table, np.int64), np.asarray(sampled_table, np.int64)
    wa, wb = [int(w) for w in enum_weights], [int(w) for w in sampled_weights]
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != len(wa) or b.shape[0] != len(wb) or a.shape[1] != b.shape[1]:
        raise ValueError(f"tables of shapes {a.shape} and {b.shape} for {len(wa)} and {len(wb)} weights")
    both = sorted(set(wa) & set(wb))
    if both:
        raise ValueError(f"weights {both} are enumerated and sampled: keep one of the two rows")
    return np.concatenate([a, b]), wa + wb


def binomial_weights(n, p):
    """B(n, w, p) = C(n, w) p^w (1 - p)^(n - w) for w = 0 .. n as float64[n + 1], through ``math.lgamma`` (n = 7776
    does not overflow)."""
    n, p = int(n), float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"p = {p} out of [0, 1]")
    out = np.zeros(n + 1)
    if p == 0.0 or p == 1.0:
        out[0 if p == 0.0 else n] = 1.0
        return out
    lp, lq, ln = math.log(p), math.log1p(-p), math.lgamma(n + 1)
    for w in range(n + 1):
        out[w] = math.exp(ln - math.lgamma(w + 1) - math.lgamma(n - w + 1) + w * lp + (n - w) * lq)
    return out


def ler_from_weights(table, weights, n, ps, exact_weights=()):
    """The logical error rate under uniform noise of rate p, for every p of ``ps``, from the counter table of a
    fixed-weight run (``run_weights``: row i = weight ``weights[i]``, [0] trials, [1] logical errors).  Returns a dict
    of float64 arrays over ``ps``:
      ``ler``      sum over the sampled w of B(n, w, p) f_w, f_w = logical_error_w / trials_w;
      ``ler_high`` ler + sum of B(n, w, p) over the weights NOT sampled: those are unknown, not assumed zero
                   (``unsampled_mass`` is that sum);
      ``stderr``   sqrt(sum of B^2 f_w (1 - f_w) / trials_w), the binomial error of the sampled part;
    and ``p`` itself.  A weight without trials counts as not sampled; a weight listed twice is a ValueError.
    ``exact_weights``: weights of ``weights`` whose row is a whole enumerated class (``run_enumerate``): f_w is exact and
    adds nothing to ``stderr``; its [0] must be C(n, w) (ValueError otherwise)."""
    table = np.asarray(table, np.int64)
    weights = check_weights(weights, n)
    exact = set(check_weights(list(exact_weights), n)) if len(exact_weights) else set()
    if not exact <= set(weights):
        raise ValueError(f"exact_weights {sorted(exact - set(weights))} are not among the weights {weights!r}")
    if table.ndim != 2 or table.shape[0] != len(weights) or table.shape[1] < 2:
        raise ValueError(f"table must have shape ({len(weights)}, {NUM_COUNTERS}), got {table.shape}")
    if len(set(weights)) != len(weights):
        raise ValueError(f"a weight is listed twice in {weights!r}")
    ps = np.atleast_1d(np.asarray(ps, np.float64))
    sampled = np.zeros(n + 1, bool)
    f = np.zeros(n + 1)
    var = np.zeros(n + 1)                      # f (1 - f) / trials
    for w, row in zip(weights, table):
        t = int(row[0])
        if w in exact and t != math.comb(n, w):
            raise ValueError(f"weight {w} is listed as exact, but its row has {t} trials, not C({n}, {w}) = {math.comb(n, w)}")
        if t > 0:
            sampled[w] = True
            f[w] = int(row[1]) / t
            var[w] = 0.0 if w in exact else f[w] * (1.0 - f[w]) / t
    out = {k: np.zeros(len(ps)) for k in ("ler", "ler_high", "stderr", "unsampled_mass")}
    out["p"] = ps
    for i, p in enumerate(ps):
        B = binomial_weights(n, p)
        out["ler"][i] = float(np.sum(B[sampled] * f[sampled]))
        out["unsampled_mass"][i] = float(np.sum(B[~sampled]))
        out["ler_high"][i] = out["ler"][i] + out["unsampled_mass"][i]
        out["stderr"][i] = math.sqrt(float(np.sum(B[sampled] ** 2 * var[sampled])))
    return out


def stabilizer_spectrum(code_names, p=0.005, trials=20000, *, max_iter=50, osd=True, **kwargs):
    """The experiment of spectrum.py:22-54: per code name the histogram int64[n + 1] of the weights of the residuals
    ``detection ^ error`` that are non-zero but logically trivial (the stabilisers BP(50) + OSD-0 leaves behind at p =
    0.005): rows 0 + 1 of ``run_spectrum``.  ``np.repeat(np.arange(n + 1), hist)`` is the script's ``weights_found``
    list, sorted.  ``kwargs`` go to ``run_spectrum``."""
    spectra = {}
    for name in code_names:
        _, weights, _ = run_spectrum(name, [p], trials, max_iter=max_iter, osd=osd, **kwargs)
        spectra[name] = weights[0, 0] + weights[0, 1]
    return spectra


REWORK_WEIGHT_LISTS = ("weights_found_BP", "weights_found_OSD", "weights_found_BP_error", "weights_found_OSD_error")


def rework_point(counters, weights, iterations):
    """One ``results[name][p]`` entry of rework/main.py:119-129 from the three outputs of a spectrum run for that
    point.  The four weight lists are expanded from the histograms with ``np.repeat``: the same multiset as the
    reference's lists, in ascending order of weight and not in trial order."""
    counters, weights, iterations = (np.asarray(a, np.int64) for a in (counters, weights, iterations))
    t = max(int(counters[0]), 1)
    max_iter = len(iterations) - 1
    its = iterations.copy()
    its[max_iter - 1] += its[max_iter]      # (an unconverged trial reports iteration index max_iter - 1)
    point = {
        "logical": int(counters[1]) / t,                                     # :114
        "osd": int(counters[6]) / t,                                         # :115 (trials BP left unconverged)
        "degeneracies": int(counters[5]) / t,                                # :116
        "average_iterations": float(np.dot(np.arange(max_iter), its[:max_iter])) / t,   # :117
        "OSD_invocation_AND_logicalError": int(counters[8]) / t,             # :118
    }
    for r, name in enumerate(REWORK_WEIGHT_LISTS):
        point[name] = np.repeat(np.arange(weights.shape[1]), weights[r]).tolist()
    return point


def rework_results(experiment, trials=10000, *, max_iter=100, osd=True, osd_method="cs", osd_order=0, osd_large=False, **kwargs):
    """The ``results[name][p]`` dictionary of rework/main.py:50-129.  ``experiment``: that script's list of {"code",
    "name", "physicalErrorRates"} dictionaries.  One ``run_spectrum`` per code (its own sampler, not numpy's stream;
    OSD-0 by default, which is what the reference's ``performOSD_enhanced`` returns on every syndrome that comes from
    an error).  The weight lists hold the reference's multisets in ascending order, not in trial order
    (``rework_point``).  ``kwargs`` go to ``run_spectrum``."""
    results = {}
    for exp in experiment:
        ps = list(exp["physicalErrorRates"])
        cnt, weights, its = run_spectrum(exp["code"], ps, trials, max_iter=max_iter, osd=osd, osd_method=osd_method,
                                         osd_order=osd_order, osd_large=osd_large, **kwargs)
        results[exp["name"]] = {p: rework_point(cnt[i], weights[i], its[i]) for i, p in enumerate(ps)}
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--code", default="[[288, 12, 18]]")
    ap.add_argument("--circuit", nargs=2, default=None, metavar=("CODE", "ROUNDS"),
                    help="circuit-level noise: the memory experiment of CODE over ROUNDS rounds, sampled and decoded on the "
                         "device (run_circuit); takes --p (every rate class), --shots N (a count here, not a file), "
                         "--basis, --no-idle, --osd*, --max-iter, --variant, --alpha, --seed, --out")
    ap.add_argument("--basis", default="Z", choices=("Z", "X"), help="--circuit: the memory basis")
    ap.add_argument("--no-idle", action="store_true", help="--circuit: no idle noise")
    ap.add_argument("--detectors", default="basis", choices=("basis", "all"),
                    help="--circuit: detectors of the memory basis only, or of both check types")
    ap.add_argument("--rates", type=float, nargs=4, default=None, metavar=("RESET", "CNOT", "IDLE", "MEAS"),
                    help="--circuit: a rate per class instead of p for every class (one --p point, which then only labels "
                         "the row)")
    ap.add_argument("--fault-weights", type=int, nargs="+", default=None, metavar="W",
                    help="--circuit: fault sets of exactly these numbers of firing fault sites instead of --p / --shots "
                         "(run_circuit_weights): a result line per weight; needs --prior-p, takes --trials, --ler-at, "
                         "--classes, --osd*, --lsd, --quant")
    ap.add_argument("--classes", nargs="+", default=None, choices=("reset", "cnot", "idle", "meas"),
                    help="--fault-weights: the rate classes whose sites can fire (default: all); the others have rate 0")
    ap.add_argument("--dem", default=None,
                    help="detector error model file (stim's text format) instead of --code / --p: run_dem")
    ap.add_argument("--phenomenological", nargs=2, default=None, metavar=("CODE", "ROUNDS"),
                    help="the phenomenological space-time model of CODE over ROUNDS rounds (dem.phenomenological) at the "
                         "one --p, data and measurement errors alike, instead of --code or --dem: run_dem; --distance "
                         "defaults to the code's")
    ap.add_argument("--window", type=int, nargs=2, default=None, metavar=("W", "F"),
                    help="with --phenomenological: the sliding-window decoder -- windows of W rounds, each commits F "
                         "(flooding BP [+ --osd]; not with --relay, --gd, --layered, --budgets, --spectrum, --weights, "
                         "--shots)")
    ap.add_argument("--distance", type=int, default=0,
                    help="with --dem: the distance of the miscorrected / incorrectable split (0: all incorrectable)")
    ap.add_argument("--p", type=float, nargs="+",
                    default=[0.05, 0.04, 0.03, 0.02, 0.01, 0.009, 0.008, 0.007])   # :39
    ap.add_argument("--shots", default=None, metavar="DETS",
                    help="with --dem: decode the RECORDED shots of this file (detection events, stim's b8 or 01 "
                         "format) instead of sampling: run_shots; prints the counters as one JSON line")
    ap.add_argument("--obs", default=None, metavar="OBS",
                    help="with --shots: the recorded observables, a file of the same format (stim's --obs_out)")
    ap.add_argument("--shots-format", choices=("b8", "01"), default="b8")
    ap.add_argument("--append-observables", action="store_true",
                    help="with --shots: every shot of DETS carries its observables behind the detection events")
    ap.add_argument("--predictions-out", default=None, metavar="PRED.npy",
                    help="with --shots: write the predictions (uint64 masks, bit l = observable l) of this rank's "
                         "shots; with several ranks the file name gets .rank<r> before its extension")
    ap.add_argument("--depolarizing", type=float, nargs="+", default=None, metavar="P",
                    help="Pauli noise of total strength P on both sectors of the code, decoded in two stages with the "
                         "second stage's prior conditioned on the first (run_depolarizing); with --osd")
    ap.add_argument("--bias", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("X", "Y", "Z"),
                    help="with --depolarizing: the proportions of X, Y and Z errors (default 1 1 1)")
    ap.add_argument("--independent", action="store_true",
                    help="with --depolarizing: decode the two sectors independently (the baseline)")
    ap.add_argument("--trials", type=int, default=10000)                          # :36
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--budgets", type=int, nargs="+", default=None,
                    help="a ladder of iteration limits decoded in ONE pass instead of --max-iter (one --p): a result "
                         "line per limit (run_budgets / run_dem_budgets)")
    ap.add_argument("--llr-hist", nargs=3, default=None, metavar=("BINS", "LO", "HI"),
                    help="with --budgets: also the histograms of BP's posterior LLRs per limit, by converged flag and "
                         "true bit, over BINS bins of [LO, HI] plus below / above / NaN columns (run_llr_hist / "
                         "run_dem_llr_hist); with --out the table goes to the .npz beside it")
    ap.add_argument("--spectrum", default=None, metavar="OUT.npz",
                    help="also collect the residual-weight spectra and the iteration histogram of every point "
                         "(run_spectrum / run_dem_spectrum) and write counters, weights, iterations to this .npz")
    ap.add_argument("--weights", type=int, nargs="+", default=None,
                    help="errors of exactly these weights instead of --p (run_weights): a result line per weight; "
                         "needs --prior-p")
    ap.add_argument("--enumerate", type=int, nargs="+", default=None, metavar="W",
                    help="decode EVERY error of these weights (run_enumerate): exact failure fractions, a result line "
                         "per weight; needs --prior-p; with --weights the two tables give one --ler-at estimate in "
                         "which the enumerated weights carry no error bar")
    ap.add_argument("--failures", default=None, metavar="OUT.npz",
                    help="with --enumerate: also write the failing patterns of every enumerated weight (ranks, kinds, "
                         "columns; enumerate.failing_patterns) to this .npz (flooding BP [+ --osd] only)")
    ap.add_argument("--failures-what", choices=("logical", "unconverged", "either"), default="logical")
    ap.add_argument("--failures-cap", type=int, default=1 << 20, metavar="N",
                    help="with --failures: keep at most N patterns per weight")
    ap.add_argument("--prior-p", type=float, default=None,
                    help="with --weights / --enumerate: the error rate the decoder's prior is built for")
    ap.add_argument("--ler-at", type=float, nargs="+", default=None, metavar="P",
                    help="with --weights / --enumerate: print the logical error rate at these p (ler_from_weights)")
    ap.add_argument("--draws", type=int, default=1, choices=(1, 2))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--variant", choices=("sum-product", "damped", "min-sum"), default="sum-product")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--damping", type=float, default=1.0)
    ap.add_argument("--clip-llr", type=float, default=20.0)
    ap.add_argument("--osd", action="store_true", help="OSD-0 on the trials BP does not converge on")
    ap.add_argument("--osd-method", choices=("cs", "e"), default="cs",
                    help="with --osd-order W >= 1: combination sweep or exhaustive search")
    ap.add_argument("--osd-order", type=int, default=0,
                    help="with --osd: order-w OSD instead of OSD-0 (cs: 1..64, e: 1..12)")
    ap.add_argument("--osd-large", action="store_true",
                    help="with --osd-order W >= 1: also on matrices beyond the one-wavefront OSD kernel (space-time "
                         "and detector-error-model matrices of up to 8192 rows)")
    ap.add_argument("--relay", type=int, nargs=2, default=None, metavar=("LEGS", "ITERS"),
                    help="Relay-BP instead of OSD on the trials BP does not converge on: LEGS legs of ITERS min-sum "
                         "iterations each (with --alpha and --clip-llr; not with --osd, --budgets, --spectrum, --shots)")
    ap.add_argument("--relay-large", action="store_true",
                    help="with --relay: also on matrices whose record state passes 160 KiB of LDS (space-time and "
                         "detector-error-model matrices): their messages live in a global workspace")
    ap.add_argument("--relay-gamma0", type=float, default=0.125, help="memory strength of leg 0, every variable")
    ap.add_argument("--relay-interval", type=float, nargs=2, default=(-0.24, 0.66), metavar=("LO", "HI"),
                    help="later legs draw a strength per variable uniformly from [LO, HI] (seeded by --seed)")
    ap.add_argument("--gd", type=int, nargs=2, default=None, metavar=("T", "ROUNDS"),
                    help="BP guided decimation on the trials BP does not converge on: rounds of T iterations, at most "
                         "ROUNDS variables decimated (with --alpha and --clip-llr; not with --osd, --relay, --budgets, "
                         "--spectrum, --shots)")
    ap.add_argument("--gd-large", action="store_true",
                    help="with --gd: also on matrices whose record state passes 160 KiB of LDS (space-time and "
                         "detector-error-model matrices): their messages live in a global workspace")
    ap.add_argument("--gd-llr", type=float, default=25.0, metavar="X", help="the prior a decimated variable gets is +-X")
    ap.add_argument("--gd-variant", choices=("sum-product", "min-sum"), default="min-sum",
                    help="the BP that --gd runs between decimations")
    ap.add_argument("--lsd", type=int, default=None, metavar="G",
                    help="localized statistics decoding on the trials BP does not converge on: every invalid cluster "
                         "activates its G least reliable neighbours per round, 0: all of them (not with --osd, --relay, "
                         "--gd, --budgets, --spectrum, --shots, --window)")
    ap.add_argument("--lsd-large", action="store_true",
                    help="with --lsd: also on matrices whose rows pass 160 KiB of LDS or number more than 2048 (space-time "
                         "and detector-error-model matrices): the rows of the active checks live in a global workspace")
    ap.add_argument("--layered", action="store_true",
                    help="BP runs the layered (check-serial) schedule in its default order instead of flooding "
                         "(sum-product or min-sum; not with --budgets, --spectrum, --shots)")
    ap.add_argument("--layered-large", action="store_true",
                    help="with --layered: also on matrices whose record state passes 160 KiB of LDS (space-time and "
                         "detector-error-model matrices): their messages live in a global workspace")
    ap.add_argument("--quant", nargs=2, default=None, metavar=("BITS", "SCALE"),
                    help="the first stage is fixed-point min-sum: messages of BITS bits (2..16), SCALE integer units per "
                         "unit of LLR (needs --variant min-sum; not with --layered, --budgets, --spectrum, --shots, "
                         "--window, --depolarizing)")
    ap.add_argument("--quant-alpha", type=int, nargs=2, default=(1, 0), metavar=("NUM", "SHIFT"),
                    help="with --quant: the normalisation NUM / 2^SHIFT (default 1 / 1)")
    ap.add_argument("--quant-beta", type=int, default=0, metavar="B", help="with --quant: the offset, in integer units")
    ap.add_argument("--relay-stop", type=int, default=1, metavar="S", help="stop after S solutions, keep the lightest")
    ap.add_argument("--out", default=None, help="write the counter table as JSON")
    ap.add_argument("--gpus", type=int, default=0,
                    help="N > 1 without a launcher: start N ranks (one per GPU) and reduce over RCCL")
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL; gloo only for rehearsals")
    ap.add_argument("--share-device", action="store_true", help="rehearsal: every rank on cuda:0")
    args = ap.parse_args(argv)
    try:
        osd_run_flags(args.osd, args.osd_method, args.osd_order, args.osd_large)
    except ValueError as e:
        ap.error(str(e))
    if args.circuit is None and (args.fault_weights is not None or args.classes is not None):
        ap.error("--fault-weights and --classes need --circuit")
    if args.circuit is not None and args.fault_weights is not None:
        if args.shots is not None or args.rates is not None:
            ap.error("--fault-weights takes --trials and --prior-p, not --shots or --rates")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--circuit runs on one GPU from the command line (mc.run_circuit_weights takes rank= and world=)")
        if args.prior_p is None or not 0.0 < args.prior_p < 1.0:
            ap.error("--fault-weights needs --prior-p in (0, 1)")
        if any(not 0.0 <= p <= 1.0 for p in args.ler_at or []):
            ap.error("--ler-at takes probabilities in [0, 1]")
        for name in ("dem", "obs", "budgets", "spectrum", "weights", "depolarizing", "relay", "gd", "layered", "window",
                     "enumerate", "phenomenological", "failures"):
            if getattr(args, name, None) not in (None, False):
                ap.error(f"--fault-weights does not combine with --{name}")
        try:
            rounds = int(args.circuit[1])
            quant = None
            if args.quant is not None:
                from . import quant as quant_mod
                quant = quant_mod.QuantConfig(int(args.quant[0]), float(args.quant[1]), tuple(args.quant_alpha),
                                              args.quant_beta)
            t0 = time.perf_counter()
            table, N = run_circuit_weights(args.circuit[0], rounds, args.fault_weights, args.trials, prior_p=args.prior_p,
                                           classes=args.classes, basis=args.basis, idle=not args.no_idle,
                                           detectors=args.detectors, seed=args.seed, max_iter=args.max_iter,
                                           variant=_VARIANTS[args.variant], alpha=args.alpha, damping=args.damping,
                                           clip_llr=args.clip_llr, osd=args.osd, osd_method=args.osd_method,
                                           osd_order=args.osd_order, osd_large=args.osd_large, lsd=args.lsd,
                                           lsd_large=args.lsd_large, quant=quant)
            result = {"circuit": args.circuit[0], "rounds": rounds, "basis": args.basis, "detectors": args.detectors,
                      "classes": args.classes, "prior_p": args.prior_p, "sites": N, "trials": args.trials,
                      "seconds": time.perf_counter() - t0,
                      "points": [dict(weight=w, **summarize(row)) for w, row in zip(args.fault_weights, table)]}
            if args.ler_at:
                est = ler_from_weights(table, args.fault_weights, N, args.ler_at)
                result["ler_at"] = {k: [float(x) for x in v] for k, v in est.items()}
        except (ValueError, KeyError) as e:
            ap.error(f"--fault-weights: {e}")
        print(json.dumps(result))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f)
        return 0
    if args.circuit is not None:
        if args.p is None or args.shots is None or not str(args.shots).isdigit():
            ap.error("--circuit needs --p and --shots N (with --circuit, --shots is a count, not a file of recorded shots)")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--circuit runs on one GPU from the command line (mc.run_circuit takes rank= and world=)")
        if args.rates is not None and len(args.p) != 1:
            ap.error("--rates needs exactly one --p point")
        for name in ("dem", "obs", "budgets", "spectrum", "weights", "depolarizing", "relay", "gd", "lsd", "layered", "quant",
                     "window", "enumerate", "phenomenological"):
            if getattr(args, name, None) not in (None, False):
                ap.error(f"--circuit does not combine with --{name}")
        try:
            rounds = int(args.circuit[1])
            table = run_circuit(args.circuit[0], rounds, args.p, int(args.shots), basis=args.basis, idle=not args.no_idle,
                                detectors=args.detectors,
                                rates=None if args.rates is None else [args.rates],
                                seed=args.seed, max_iter=args.max_iter, alpha=args.alpha,
                                variant=_VARIANTS[args.variant], damping=args.damping, clip_llr=args.clip_llr,
                                osd=args.osd, osd_method=args.osd_method, osd_order=args.osd_order,
                                osd_large=args.osd_large)
        except (ValueError, KeyError) as e:
            ap.error(f"--circuit: {e}")
        result = {"circuit": args.circuit[0], "rounds": rounds, "basis": args.basis, "detectors": args.detectors,
                  "rates": args.rates, "shots": int(args.shots),
                  "points": [dict(p=p, **summarize(row)) for p, row in zip(args.p, table)]}
        print(json.dumps(result))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f)
        return 0
    for name in ("relay", "gd", "layered"):
        if getattr(args, name + "_large") and getattr(args, name) in (None, False):
            ap.error(f"--{name}-large needs --{name}")
    relay = None
    if args.relay is not None:
        if args.osd:
            ap.error("--relay and --osd exclude each other")
        if args.budgets is not None or args.spectrum is not None or args.shots is not None:
            ap.error("--relay does not combine with --budgets, --spectrum or --shots")
        relay = dict(legs=args.relay[0], iters=args.relay[1], gamma0=args.relay_gamma0,
                     interval=tuple(args.relay_interval), seed=args.seed, stop_after=args.relay_stop, alpha=args.alpha,
                     clip_llr=args.clip_llr, large=args.relay_large)
        try:
            from . import relay as relay_mod
            relay_mod.as_config(relay, 1)
        except (ValueError, TypeError) as e:
            ap.error(f"--relay: {e}")
    gd = None
    if args.gd is not None:
        if args.osd or args.relay is not None:
            ap.error("--gd excludes --osd and --relay")
        if args.budgets is not None or args.spectrum is not None or args.shots is not None:
            ap.error("--gd does not combine with --budgets, --spectrum or --shots")
        gd = dict(iters_per_round=args.gd[0], max_rounds=args.gd[1], decim_llr=args.gd_llr,
                  variant=_lib.MIN_SUM if args.gd_variant == "min-sum" else _lib.SUM_PRODUCT, alpha=args.alpha,
                  clip_llr=args.clip_llr, large="auto" if args.gd_large else False)
        try:
            from . import gd as gd_mod
            gd_mod.as_config(gd)
        except (ValueError, TypeError) as e:
            ap.error(f"--gd: {e}")
    lsd = None
    if args.lsd_large and args.lsd is None:
        ap.error("--lsd-large needs --lsd")
    if args.lsd is not None:
        if args.osd or args.relay is not None or args.gd is not None:
            ap.error("--lsd excludes --osd, --relay and --gd")
        if (args.budgets is not None or args.spectrum is not None or args.shots is not None
                or getattr(args, "window", None) is not None):
            ap.error("--lsd does not combine with --budgets, --spectrum, --shots or --window")
        try:
            from . import lsd as lsd_mod
            lsd = lsd_mod.check_bits_per_step(args.lsd)
        except ValueError as e:
            ap.error(f"--lsd: {e}")
    if args.layered:
        if args.budgets is not None or args.spectrum is not None or args.shots is not None:
            ap.error("--layered does not combine with --budgets, --spectrum or --shots")
        if args.variant == "damped":
            ap.error("--layered needs --variant sum-product or min-sum")
        if args.layered_large:
            args.layered = "large"          # (the drivers' layered= argument: True or "large")
    quant = None
    if args.quant is not None:
        if (args.layered or args.budgets is not None or args.spectrum is not None or args.shots is not None
                or args.window is not None or args.depolarizing is not None):
            ap.error("--quant does not combine with --layered, --budgets, --spectrum, --shots, --window or --depolarizing")
        if args.variant != "min-sum":
            ap.error("--quant needs --variant min-sum")
        try:
            from . import quant as quant_mod
            quant = quant_mod.QuantConfig(int(args.quant[0]), float(args.quant[1]), tuple(args.quant_alpha),
                                          args.quant_beta)
        except ValueError as e:
            ap.error(f"--quant: {e}")
    if args.depolarizing is not None:
        if (args.dem is not None or args.phenomenological is not None or args.shots is not None or args.budgets is not None
                or args.spectrum is not None or args.weights is not None or relay is not None or gd is not None
                or lsd is not None or args.layered):
            ap.error("--depolarizing combines with --osd only")
        if args.variant == "damped":
            ap.error("--depolarizing needs --variant sum-product or min-sum")
        try:
            for p in args.depolarizing:
                pauli_rates(p, args.bias)
        except ValueError as e:
            ap.error(f"--depolarizing: {e}")
    if args.budgets is not None:
        try:
            _lib.check_budgets(args.budgets)
        except ValueError as e:
            ap.error(f"--budgets: {e}")
        if args.dem is None and len(args.p) != 1:
            ap.error("--budgets takes one --p")
    if args.llr_hist is not None:
        if args.budgets is None:
            ap.error("--llr-hist needs --budgets")
        try:
            args.llr_hist = _lib.check_llr_hist(int(args.llr_hist[0]), float(args.llr_hist[1]), float(args.llr_hist[2]),
                                                len(args.budgets))
        except ValueError as e:
            ap.error(f"--llr-hist: {e}")
    if args.spectrum is not None:
        if args.budgets is not None:
            ap.error("--spectrum does not combine with --budgets")
        if not 1 <= args.max_iter <= _lib.MC_SPECTRUM_MAX_ITER:
            ap.error(f"--spectrum takes --max-iter in [1, {_lib.MC_SPECTRUM_MAX_ITER}]")
    if args.weights is not None or args.enumerate is not None:
        if args.dem is not None or args.budgets is not None or args.spectrum is not None or args.shots is not None:
            ap.error("--weights / --enumerate do not combine with --dem, --budgets, --spectrum or --shots")
        if args.prior_p is None or not 0.0 < args.prior_p < 1.0:
            ap.error("--weights / --enumerate need --prior-p in (0, 1)")
        if any(not 0.0 <= p <= 1.0 for p in args.ler_at or []):
            ap.error("--ler-at takes probabilities in [0, 1]")
        try:
            n_code = codes.load_code(args.code).n
            listed = check_weights((args.weights or []) + (args.enumerate or []), n_code)
            if len(set(listed)) != len(listed):
                raise ValueError("a weight is listed twice")
            if args.enumerate is not None:
                from . import enumerate as enum_mod
                for w in args.enumerate:
                    enum_mod.count(n_code, w)
        except ValueError as e:
            ap.error(f"--weights / --enumerate: {e}")
        if args.enumerate is not None and (args.depolarizing is not None or args.phenomenological is not None
                                           or args.window is not None):
            ap.error("--enumerate does not combine with --depolarizing, --phenomenological or --window")
        if args.failures is not None and (args.enumerate is None or relay is not None or gd is not None or lsd is not None
                                          or args.layered or quant is not None):
            ap.error("--failures needs --enumerate and flooding BP [+ --osd] (not --relay, --gd, --lsd, --layered, --quant)")
        if args.failures_cap < 0:
            ap.error("--failures-cap must be >= 0 (with --enumerate)")
    elif args.prior_p is not None or args.ler_at is not None or args.failures is not None:
        ap.error("--prior-p, --ler-at and --failures need --weights or --enumerate")
    dem_model = None
    if args.dem is not None:
        from . import dem
        if not os.path.isfile(args.dem):
            ap.error(f"--dem {args.dem}: no such file")
        try:
            dem_model = dem.load_dem(args.dem)
        except ValueError as e:
            ap.error(f"--dem {args.dem}: {e}")
        if dem_model[1].shape[0] > 64:
            ap.error(f"--dem {args.dem}: {dem_model[1].shape[0]} observables (at most 64)")

    check_round, model_name = None, args.dem
    if args.phenomenological is not None:
        from . import dem, window as window_mod
        if args.dem is not None or args.shots is not None or args.weights is not None:
            ap.error("--phenomenological does not combine with --dem, --shots or --weights")
        if len(args.p) != 1:
            ap.error("--phenomenological takes one --p")
        code_name, rounds = args.phenomenological
        try:
            rounds = int(rounds)
            code = codes.load_code(code_name)
            dem_model = dem.phenomenological(code, rounds, args.p[0])
            check_round = window_mod.phenomenological_rounds(code, rounds)
        except (ValueError, KeyError, OSError) as e:
            ap.error(f"--phenomenological {code_name} {rounds}: {e}")
        if args.distance == 0 and code.distance:
            args.distance = int(code.distance)
        model_name = f"phenomenological {code_name} x {rounds}, p={args.p[0]}"
    if args.window is not None:
        if check_round is None:
            ap.error("--window needs --phenomenological (a detector error model file does not say its rounds)")
        if (relay is not None or gd is not None or args.layered or args.budgets is not None or args.spectrum is not None
                or args.weights is not None or args.shots is not None):
            ap.error("--window does not combine with --relay, --gd, --layered, --budgets, --spectrum, --weights or --shots")
        if args.window[0] < 1 or not 1 <= args.window[1] <= args.window[0]:
            ap.error("--window W F needs W >= 1 and 1 <= F <= W")

    shot_data = None
    if args.shots is not None:
        from . import shots as shots_mod
        if dem_model is None:
            ap.error("--shots needs --dem")
        if args.budgets is not None or args.spectrum is not None:
            ap.error("--shots does not combine with --budgets or --spectrum")
        if args.obs is not None and args.append_observables:
            ap.error("--obs and --append-observables exclude each other")
        for path in (args.shots, args.obs):
            if path is not None and not os.path.isfile(path):
                ap.error(f"{path}: no such file")
        if dem_model[1].shape[0] < 1:
            ap.error(f"--dem {args.dem}: no observables to predict")
        try:
            shot_data = shots_mod.read_shots(
                args.shots, dem_model[0].shape[0],
                dem_model[1].shape[0] if (args.obs is not None or args.append_observables) else 0,
                args.shots_format, obs=args.obs)
        except ValueError as e:
            ap.error(f"--shots: {e}")
    elif args.obs is not None or args.predictions_out is not None or args.append_observables:
        ap.error("--obs, --append-observables and --predictions-out need --shots")

    import sys
    from . import launch
    if argv is None:          # (a caller passing argv runs in-process, whatever --gpus says)
        launch.maybe_self_launch(args.gpus, ["-m", "qldpc_amd.mc"] + sys.argv[1:])

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = 0 if args.share_device else int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher set WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.backend)
    common = dict(draws=args.draws, seed=args.seed, max_iter=args.max_iter, variant=_VARIANTS[args.variant],
                  alpha=args.alpha, damping=args.damping, clip_llr=args.clip_llr, osd=args.osd,
                  osd_method=args.osd_method, osd_order=args.osd_order, osd_large=args.osd_large, device=local)
    stages = dict(relay=relay, layered=args.layered, gd=gd, lsd=lsd, lsd_large=args.lsd_large, quant=quant)
    if args.depolarizing is not None:
        kw = {k: common[k] for k in ("seed", "max_iter", "variant", "alpha", "damping", "clip_llr", "osd", "osd_method",
                                     "osd_order", "device")}
        t0 = time.perf_counter()
        table = run_depolarizing(args.code, args.depolarizing, args.trials, bias=tuple(args.bias),
                                 correlated=not args.independent, rank=rank, world=world, **kw)
        dt = time.perf_counter() - t0
        if rank == 0:
            rows = ("sector_a", "sector_b", "joint")
            result = {"code": args.code, "depolarizing": list(args.depolarizing), "bias": list(args.bias),
                      "correlated": not args.independent, "trials": args.trials, "max_iter": args.max_iter,
                      "variant": args.variant, "osd": args.osd, "world_size": world, "seconds": dt,
                      "points": [{"p": p, **{name: {k: int(v) for k, v in zip(_lib.COUNTER_NAMES, row)}
                                             for name, row in zip(rows, point)},
                                  "ler": int(point[2][1]) / max(int(point[2][0]), 1)}
                                 for p, point in zip(args.depolarizing, table)]}
            print(json.dumps(result))
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    if shot_data is not None:
        H, L, probs = dem_model
        kw = {k: common[k] for k in ("max_iter", "variant", "alpha", "damping", "clip_llr", "osd", "osd_method",
                                     "osd_order", "osd_large", "device")}
        t0 = time.perf_counter()
        cnt, pred, conv = run_shots(H, L, shot_data[0], shot_data[1], prior=dem_prior(probs), rank=rank, world=world,
                                    **kw)
        dt = time.perf_counter() - t0
        if args.predictions_out:
            out = args.predictions_out
            if world > 1:
                root, ext = os.path.splitext(out)
                out = f"{root}.rank{rank}{ext}"
            with open(out, "wb") as f:       # (np.save on a name would append .npy to other extensions)
                np.save(f, pred)
        if rank == 0:
            result = {"dem": args.dem, "shots": args.shots, "m": int(H.shape[0]), "n": int(H.shape[1]),
                      "k": int(L.shape[0]), "observables": shot_data[1] is not None, "max_iter": args.max_iter,
                      "variant": args.variant, "osd": args.osd, "osd_method": args.osd_method,
                      "osd_order": args.osd_order, "world_size": world, "seconds": dt,
                      "counters": {k: int(v) for k, v in zip(_lib.COUNTER_NAMES, cnt)}}
            print(json.dumps(result))
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    if args.enumerate is not None:
        from . import bp, enumerate as enum_mod
        kw = {k: v for k, v in common.items() if k not in ("draws", "seed")}
        code = codes.load_code(args.code)
        t0 = time.perf_counter()
        table = run_enumerate(args.code, args.enumerate, prior_p=args.prior_p, rank=rank, world=world, **stages, **kw)
        dt = time.perf_counter() - t0
        weights, exact = list(args.enumerate), list(args.enumerate)
        if args.weights is not None:       # sampled weights beside the enumerated ones: one table for the LER
            sampled = run_weights(args.code, args.weights, args.trials, prior_p=args.prior_p, seed=args.seed, rank=rank,
                                  world=world, **stages, **kw)
            table, weights = merge_weight_tables(table, exact, sampled, args.weights)
        failures = {}
        if args.failures is not None and rank == 0:      # (one GPU: a class this small needs no more)
            fkw = {k: kw[k] for k in ("max_iter", "variant", "alpha", "damping", "clip_llr", "osd", "osd_method",
                                      "osd_order", "osd_large", "device")}
            for w in exact:
                f = enum_mod.failing_patterns(code.Hx, code.Lx, w, prior=prior_of(args.prior_p, code.n),
                                              what=args.failures_what, cap=args.failures_cap, **fkw)
                failures.update({f"ranks_w{w}": f["ranks"], f"kinds_w{w}": f["kinds"], f"columns_w{w}": f["columns"],
                                 f"found_w{w}": np.int64(f["found"])})
                print(f"  weight={w}: {f['found']} failing patterns ({args.failures_what}), {len(f['ranks'])} kept")
            np.savez(args.failures, weights=np.asarray(exact, np.int64), what=args.failures_what, **failures)
            print(f"failing patterns written to {args.failures}")
        if rank == 0:
            rows, ler_rows = [], []
            for w, row in zip(weights, table):
                s = summarize(row)
                s.update(weight=w, prior_p=args.prior_p, exact=w in exact)
                rows.append(s)
                print(f"  weight={w} ({'all ' + str(int(row[0])) + ' patterns' if w in exact else 'sampled'}): "
                      f"f_w={s['ler']:.6e}, BP-only f_w={s['ler_bp_only']:.6e}, not converged={s['not_converged']}")
            done = sum(int(table[i][0]) for i, w in enumerate(weights) if w in exact)
            print(f"{len(exact)} weight classes, {done} patterns on {world} GPU(s): {dt:.3f} s")
            if args.ler_at:
                est = ler_from_weights(table, weights, code.n, args.ler_at, exact_weights=exact)
                for i, p in enumerate(args.ler_at):
                    ler_rows.append({k: float(est[k][i]) for k in ("p", "ler", "ler_high", "stderr", "unsampled_mass")})
                    print(f"  p={p}: LER={est['ler'][i]:.6e} +- {est['stderr'][i]:.1e} (at most {est['ler_high'][i]:.6e}: "
                          f"the weights not covered carry {est['unsampled_mass'][i]:.3e})")
            if args.out:
                with open(args.out, "w") as f:
                    json.dump({"code": args.code, "enumerate": exact, "weights": args.weights, "prior_p": args.prior_p,
                               "trials": args.trials, "max_iter": args.max_iter, "variant": args.variant, "osd": args.osd,
                               "osd_method": args.osd_method, "osd_order": args.osd_order, "world_size": world,
                               "seconds": dt, "points": rows, "ler": ler_rows}, f, indent=1)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    if args.budgets is not None:
        points = list(args.budgets)      # one row per iteration limit
        del common["max_iter"]

        llr_tables = {}                  # table and edges of the last sweep (the timed one)

        def sweep(trials, ps, rank, world):          # (the whole ladder, also for the warm-up)
            if args.llr_hist is not None:
                bins, lo, hi = args.llr_hist
                if dem_model is None:
                    cnt, llr_tables["hist"], llr_tables["edges"] = run_llr_hist(
                        args.code, args.p[0], trials, points, bins, (lo, hi), rank=rank, world=world, **common)
                else:
                    cnt, llr_tables["hist"], llr_tables["edges"] = run_dem_llr_hist(
                        *dem_model, trials, points, bins, (lo, hi), distance=args.distance, rank=rank, world=world,
                        **common)
                return cnt
            if dem_model is None:
                return run_budgets(args.code, args.p[0], trials, points, rank=rank, world=world, **common)
            return run_dem_budgets(*dem_model, trials, points, distance=args.distance, rank=rank, world=world, **common)
    elif args.spectrum is not None:
        points = args.p if dem_model is None else [None]
        tables = {}                      # weights and iterations of the last sweep (the timed one)

        def sweep(trials, ps, rank, world):
            if dem_model is None:
                cnt, tables["weights"], tables["iterations"] = run_spectrum(args.code, ps, trials, rank=rank,
                                                                            world=world, **common)
            else:
                cnt, tables["weights"], tables["iterations"] = run_dem_spectrum(
                    *dem_model, trials, distance=args.distance, rank=rank, world=world, **common)
            return cnt
    elif args.weights is not None:
        points = list(args.weights)      # one row per weight
        del common["draws"]

        def sweep(trials, ps, rank, world):
            return run_weights(args.code, ps, trials, prior_p=args.prior_p, rank=rank, world=world, **stages, **common)
    elif dem_model is None:
        points = args.p

        def sweep(trials, ps, rank, world):
            return run_sweep(args.code, ps, trials, rank=rank, world=world, **stages, **common)
    else:
        points = [None]                  # one point: the model's own probabilities

        def sweep(trials, ps, rank, world):
            return run_dem(*dem_model, trials, distance=args.distance, rank=rank, world=world, window=args.window,
                           check_round=check_round, **stages, **common)[None, :]
    # one-time setup, timed apart from the sweep: HIP context, the decoder of this code (tables, device
    # buffers, kernel images) and a first small launch of the kernels the sweep uses (0.3 - 0.4 s)
    t0 = time.perf_counter()
    sweep(min(args.trials, 4096), points[:1], 0, 1)
    t_setup = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    t0 = time.perf_counter()
    table = sweep(args.trials, points, rank, world)
    dt = time.perf_counter() - t0
    if rank == 0:
        rows = []
        for p, row in zip(points, table):
            s = summarize(row)
            if args.budgets is not None:
                s["max_iter"] = p
                if dem_model is None:
                    s["p"] = args.p[0]
                    label = f"p={args.p[0]}, max_iter={p}"
                else:
                    s.update(dem=model_name)
                    label = f"dem={model_name}, max_iter={p}"
            elif args.weights is not None:
                s.update(weight=p, prior_p=args.prior_p)
                label = f"weight={p}"
            elif dem_model is None:
                s["p"] = p
                label = f"p={p}"
            else:
                H, L, probs = dem_model
                s.update(dem=model_name, m=int(H.shape[0]), n=int(H.shape[1]), k=int(L.shape[0]))
                if args.window is not None:
                    s.update(window=list(args.window))
                label = f"dem={model_name} ({H.shape[0]} x {H.shape[1]}, k={L.shape[0]})"
            rows.append(s)
            print(f"  {label}: LER={s['ler']:.6f}, BP-only LER={s['ler_bp_only']:.6f}, "
                  f"degeneracies={s['degenerateErrors']}, not converged={s['not_converged']}, "
                  f"mean iters={s['mean_iterations']:.2f}")
        if args.budgets is not None:
            print(f"{len(points)} iteration limits, one pass over {args.trials} trials on {world} GPU(s): {dt:.3f} s "
                  f"({args.trials / dt:.3e} trials/s); one-time setup {t_setup:.2f} s")
        else:
            print(f"{len(points)} points x {args.trials} trials on {world} GPU(s): {dt:.3f} s "
                  f"({len(points) * args.trials / dt:.3e} trials/s); one-time setup {t_setup:.2f} s")
        ler_rows = []
        if args.weights is not None and args.ler_at:
            est = ler_from_weights(table, points, codes.load_code(args.code).n, args.ler_at)
            for i, p in enumerate(args.ler_at):
                ler_rows.append({k: float(est[k][i]) for k in ("p", "ler", "ler_high", "stderr", "unsampled_mass")})
                print(f"  p={p}: LER={est['ler'][i]:.6e} +- {est['stderr'][i]:.1e} (at most {est['ler_high'][i]:.6e}: "
                      f"the weights not sampled carry {est['unsampled_mass'][i]:.3e})")
        if args.spectrum is not None:
            np.savez(args.spectrum, counters=table, weights=tables["weights"], iterations=tables["iterations"],
                     p=np.asarray([np.nan if p is None else p for p in points], np.float64))
            print(f"spectra written to {args.spectrum}: weights {tables['weights'].shape}, "
                  f"iterations {tables['iterations'].shape}")
        if args.llr_hist is not None:
            h = llr_tables["hist"]
            print(f"posterior-LLR histograms {h.shape}: {int(h.sum())} values, {int(h[:, :, 1:-2].sum())} inside "
                  f"[{args.llr_hist[1]}, {args.llr_hist[2]}], {int(h[:, :, -1].sum())} NaN")
            if args.out:
                npz = os.path.splitext(args.out)[0] + ".npz"
                np.savez(npz, counters=table, llr_hist=h, llr_edges=llr_tables["edges"], budgets=np.asarray(points))
                print(f"LLR histograms written to {npz}")
        if args.out:
            with open(args.out, "w") as f:
                model = {"code": args.code} if dem_model is None else {"dem": model_name, "distance": args.distance}
                if args.window is not None:
                    model["window"] = list(args.window)
                if args.budgets is not None:
                    model["budgets"] = points
                if args.weights is not None:
                    model.update(weights=points, prior_p=args.prior_p, ler=ler_rows)
                json.dump({**model, "trials": args.trials, "max_iter": points[-1] if args.budgets else args.max_iter,
                           "draws": args.draws, "seed": args.seed, "variant": args.variant,
                           "osd": args.osd, "osd_method": args.osd_method, "osd_order": args.osd_order,
                           "world_size": world, "seconds": dt, "setup_seconds": t_setup, "points": rows},
                          f, indent=1)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
