"""Sharding helpers for one-process-per-GPU runs (torch.distributed; RCCL on GPUs, gloo in the CPU tests).

Parity mode needs no collective: chains are independent (reference src/sampler.rs:1105-1126) and the chain RNG
depends only on (seed, global chain id), so a rank just owns a contiguous block of chain ids.

OPT-IN pooled adaptation (north_star's "RCCL cross-chain Welford reduction").  It is NOT reference
behaviour — every reference chain adapts alone (src/adapt_strategy.rs:24-39) — and it changes results, so it is a
separate driver, `pooled_warmup`, never the default.  All chains of all ranks share ONE diagonal transformation:
the engine runs with the transformation frozen (its own mass-matrix adaptation off, step size adapting per chain as
usual), records draws and gradients of a window in device buffers, each rank reduces its chains' window to
(count, mean[D], M2[D]) for draws and for gradients with the engine's reduction kernel (nm_pooled_partials: only healthy
chains' `is_good` draws count, like the reference's collector), the ranks exchange those 2 (2 D + 1) doubles with
ONE all_gather per window (torch.distributed: RCCL over xGMI with the nccl backend, issued on a side stream so the next
window's kernel is already running; gloo in the tests), merge them in rank order with Chan's formula, and every rank
sets sigma = (var_x / var_g)^(1/4), mean = x_bar + sigma^2 g_bar (the reference's diagonal estimate,
src/transform/diagonal.rs:107-131) for all its chains with one upload and one scatter kernel (nm_engine_set_transform).
`pooled_welford` is the merge with numpy arrays (pinned by tests/test_distributed_cpu.py).
"""
import numpy as np


def shard_chains(n_chains_total, world_size, rank):
    """Contiguous block partition: returns (chain_id_offset, n_local).  Remainder chains go to the low ranks."""
    base, rem = divmod(n_chains_total, world_size)
    n_local = base + (1 if rank < rem else 0)
    offset = rank * base + min(rank, rem)
    return offset, n_local


def welford_partial(x):
    """(count, mean, M2) of the rows of x ([n, D])."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.mean(axis=0) if n else np.zeros(x.shape[1])
    m2 = ((x - mean) ** 2).sum(axis=0) if n else np.zeros(x.shape[1])
    return float(n), mean, m2


def chan_merge(a, b):
    """Chan et al. pairwise merge of two (count, mean, M2) triples."""
    na, ma, sa = a
    nb, mb, sb = b
    n = na + nb
    if n == 0:
        return 0.0, ma, sa
    d = mb - ma
    return n, ma + d * (nb / n), sa + sb + d * d * (na * nb / n)


def pooled_welford(local, dist=None):
    """all_gather the per-rank triples (payload 2D+1 doubles per rank) and merge them in rank order."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return local
    import torch
    n, mean, m2 = local
    payload = torch.from_numpy(np.concatenate([[n], mean, m2]))
    gathered = [torch.empty_like(payload) for _ in range(dist.get_world_size())]
    dist.all_gather(gathered, payload)
    d = len(mean)
    out = None
    for g in gathered:
        g = g.numpy()
        t = (float(g[0]), g[1:1 + d].copy(), g[1 + d:].copy())
        out = t if out is None else chan_merge(out, t)
    return out


def _partials_device(pos, grad, stats, stream):
    """[2][1 + 2 D] = (count, mean[D], M2[D]) of the window's draws and gradients, by the engine's own reduction kernel
    (nm_pooled_partials, csrc/pooled_reduce.hip) on `stream`: rows of stopped chains and draws the reference's collector
    would not keep (not `is_good`) are left out."""
    import torch
    from . import _lib
    w, nc, dim = pos.shape
    out = torch.empty((2, 1 + 2 * dim), dtype=torch.float64, device=pos.device)
    _lib.check_status(_lib.load().nm_pooled_partials(w * nc, dim, pos.data_ptr(), grad.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                                     stream.cuda_stream), _lib.load().nm_pooled_last_error)
    return out


def _merge_payloads(payloads, d):
    """Chan merge of gathered [count, mean[D], M2[D]] payloads in rank order (torch tensors on one device)."""
    n, mean, m2 = payloads[0][0], payloads[0][1:1 + d], payloads[0][1 + d:]
    for p in payloads[1:]:
        nb, mb, sb = p[0], p[1:1 + d], p[1 + d:]
        if float(nb) == 0.0:            # a rank whose chains kept no draw in this window (all stopped / diverging): nothing to merge,
            continue                    # and 0 / 0 below would poison the mean (the device merge skips empty partials too)
        if float(n) == 0.0:
            n, mean, m2 = nb, mb, sb
            continue
        tot = n + nb
        delta = mb - mean
        mean = mean + delta * (nb / tot)
        m2 = m2 + sb + delta * delta * (n * nb / tot)
        n = tot
    return n, mean, m2


def window_schedule(num_tune):
    """The draw counts of the pooled drivers' windows: the reference's schedule shape — 10-draw windows in the first 30 %, then 80
    growing by 1.5x, none in the last 15 % where only the step size adapts."""
    early_end, final = int(0.3 * num_tune), num_tune - int(0.15 * num_tune)
    windows, t, w = [], 0, 80
    while t + 10 <= early_end:
        windows.append(10); t += 10
    while t + w <= final:
        windows.append(w); t += w; w = max(w + 1, int(round(w * 1.5)))
    return windows


def pooled_warmup(batch, num_tune, dist=None, windows=None, collective_device=None, on_window=None):
    """Warm up `batch` (a ChainBatch created from LowRankNutsSettings(freeze_transform=True, num_tune=num_tune)) with ONE
    diagonal transformation pooled over all chains of all ranks.  Returns the list of (draw index, sigma, mean) updates.

    windows: draw counts of the successive windows (default: the reference's schedule shape — 10-draw windows in the
    first 30 %, then 80 growing by 1.5x, none in the last 15 % where only the step size adapts).
    dist: an initialised torch.distributed module or None (single process).  With the nccl backend the payload stays on
    the GPU (RCCL); with gloo (tests) it goes through the host (`collective_device="cpu"`)."""
    import torch
    dim, nc = batch.logp.dim, batch.n_chains
    if windows is None:
        windows = window_schedule(num_tune)
    dev = torch.device("cuda", torch.cuda.current_device())
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    cdev = torch.device(collective_device) if collective_device else dev
    side = torch.cuda.Stream(device=dev)
    updates, done, pending = [], 0, None

    def finish(p):
        work, gathered, at = p
        if work is not None:
            work.wait()
        with torch.cuda.stream(side):
            # the merge of the gathered partials in rank order + the pooled transformation: the engine's own kernel (nm_pooled_finish,
            # csrc/pooled_reduce.hip — what a host without Python calls after nm_pooled_exchange)
            allp = torch.stack([g.to(dev) for g in gathered]).contiguous()
            sigma = torch.empty(dim, dtype=torch.float64, device=dev)
            mean = torch.empty(dim, dtype=torch.float64, device=dev)
            cnt = torch.zeros(1, dtype=torch.float64, device=dev)
            from . import _lib
            _lib.check_status(_lib.load().nm_pooled_finish(len(gathered), dim, allp.data_ptr(), sigma.data_ptr(), mean.data_ptr(), cnt.data_ptr(),
                                                           side.cuda_stream), _lib.load().nm_pooled_last_error)
        side.synchronize()
        if float(cnt.item()) < 3.0:     # fewer than three pooled draws: no estimate (a RunningVariance asserts count > 1,
            return                      # adapt/diagonal.rs:48; with 2 the ratio of variances is noise) — keep the current transformation
        s_h, m_h = sigma.cpu().numpy(), mean.cpu().numpy()
        batch.set_transform(s_h, m_h, np.zeros(0), np.zeros((0, dim)), np.zeros(dim))
        updates.append((at, s_h, m_h))
        if on_window:
            on_window(at, s_h, m_h)

    from .sampler import STATS_DTYPE
    for w in windows:
        pos = torch.empty((w, nc, dim), dtype=torch.float64, device=dev)
        grad = torch.empty((w, nc, dim), dtype=torch.float64, device=dev)
        # zero-filled statistics: a chain that has stopped writes no rows, and an all-zero row is not a draw the collector keeps
        stats = torch.zeros((w, nc, STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()       # (the fill runs on torch's stream, the engine on its own)
        batch.draw_device_ex(w, positions=pos.data_ptr(), stats=stats.data_ptr(), gradient=grad.data_ptr())     # the window's kernel
        if pending is not None:                # the previous window's exchange ran beside this kernel; apply it now:
            finish(pending)                    # the pooled transformation lags the draws by ONE window (documented, deliberate)
        done += w
        with torch.cuda.stream(side):          # this window's partials + the collective, off the engine's stream
            for t in (pos, grad, stats):
                t.record_stream(side)
            payload = _partials_device(pos, grad, stats, side).reshape(-1).to(cdev)
            gathered = [torch.empty_like(payload) for _ in range(world)]
            if world > 1:
                work = dist.all_gather(gathered, payload, async_op=True)
            else:
                gathered, work = [payload], None
        pending = (work, gathered, done)
    if pending is not None:
        finish(pending)
    if done < num_tune:
        batch.draw_device(num_tune - done)     # the final window: step size only (reference adapt_strategy.rs:215-221)
    return updates


# ---- the pooled LOW-RANK transformation ---------------------------------------------------------------------------
# The reference's low-rank estimate (src/transform/adapt/low_rank.rs:73-262) depends on a window of draws and gradients only through
# its count, the two means and the two centred scatter matrices sum (x - x_bar)(x - x_bar)', sum (g - g_bar)(g - g_bar)': with many
# chains the pooled window has far more rows than dimensions, the subspace the reference projects on is the whole space, and the
# projection is the identity up to a rotation that the result does not depend on.  The scatter matrices are nm_pooled_scatter's
# (csrc/pooled_scatter.hip, the f64 matrix cores); the dim x dim decompositions below cost milliseconds on the host (dim <= 1024).

def scatter_merge(a, b):
    """Chan's merge of two (count, mean[D], S[D][D]) triples of disjoint sets of rows, S the scatter matrix about the set's own mean:
    S = S_a + S_b + (n_a n_b / n) delta delta', delta = mean_b - mean_a.  (What a driver over several ranks does with the ranks' triples.)"""
    na, ma, sa = a
    nb, mb, sb = b
    ma, mb, sa, sb = (np.asarray(v, dtype=np.float64) for v in (ma, mb, sa, sb))
    if nb == 0:
        return float(na), ma, sa
    if na == 0:
        return float(nb), mb, sb
    n = float(na) + float(nb)
    d = mb - ma
    return n, ma + d * (nb / n), sa + sb + np.outer(d, d) * (na * nb / n)


def _spd_mean(cov_draws, cov_grads):
    """The SPD geometric mean as the reference forms it (adapt/low_rank.rs:262-290): G^-1/2 (G^1/2 D G^1/2)^1/2 G^-1/2."""
    w, u = np.linalg.eigh(cov_grads)
    g_sqrt = (u * np.sqrt(w)) @ u.T
    mw, mu = np.linalg.eigh(g_sqrt @ cov_draws @ g_sqrt)
    m_sqrt = (mu * np.sqrt(mw)) @ mu.T
    g_inv_sqrt = (u * (1.0 / np.sqrt(w))) @ u.T
    return g_inv_sqrt @ m_sqrt @ g_inv_sqrt


def lowrank_from_moments(count, mean_x, S_x, mean_g, S_g, gamma, eigval_cutoff, rank_multiple=1, max_rank=None):
    """The reference's low-rank estimate (`compute_update`) from the moments of a window: count, the means of draws and gradients and
    their centred scatter matrices (SUMS, as in the reference, which does not divide by n).  Returns (stds, mean, vals, vecs [n_eig][dim],
    mu_low_rank) — what ChainBatch.set_transform takes — or None when anything is not finite or count < 3.

    sigma = (S_x_dd / S_g_dd)^(1/4); mean = x_bar + sigma^2 g_bar; with D = diag(sigma): A = D^-1 S_x D^-1 / gamma + I,
    B = D S_g D / gamma + I, their SPD geometric mean, its eigenpairs with lambda > cutoff or lambda < 1 / cutoff, and
    mu_low_rank = dm + gm + U ((lambda - 1) . U' gm) for the rescaled means dm = (x_bar - mean) / sigma, gm = g_bar sigma.
    rank_multiple = m > 1: the kept set is rounded up to the next multiple of m (at most dim) by keeping the next eigenpairs in order
    of |ln lambda| WITH THEIR OWN lambda — a strictly closer approximation of the geometric mean than dropping them, and what makes the
    result eligible for the matrix-core kernels (dim and rank multiples of 8).
    max_rank (an engine's lowrank_max_rank): at most that many pairs are returned — the largest multiple of m that fits (max_rank itself
    where none does), the pairs of largest |ln lambda|; the ones left out are treated as 1, as the cutoff treats the rest."""
    mean_x, mean_g = np.asarray(mean_x, dtype=np.float64), np.asarray(mean_g, dtype=np.float64)
    S_x, S_g = np.asarray(S_x, dtype=np.float64), np.asarray(S_g, dtype=np.float64)
    dim = mean_x.shape[0]
    if not (count >= 3) or not all(np.isfinite(v).all() for v in (mean_x, mean_g, S_x, S_g)):
        return None
    with np.errstate(all="ignore"):
        sigma = np.sqrt(np.sqrt(np.diag(S_x) / np.diag(S_g)))
        mean = mean_x + sigma * sigma * mean_g
        dm, gm = (mean_x - mean) * (1.0 / sigma), mean_g * sigma
        a = S_x * np.outer(1.0 / sigma, 1.0 / sigma) * (1.0 / gamma)
        b = S_g * np.outer(sigma, sigma) * (1.0 / gamma)
    if not (np.isfinite(sigma).all() and (sigma > 0).all() and np.isfinite(a).all() and np.isfinite(b).all()):
        return None
    a[np.diag_indices(dim)] += 1.0
    b[np.diag_indices(dim)] += 1.0
    try:
        with np.errstate(all="ignore"):
            gmean = _spd_mean((a + a.T) * 0.5, (b + b.T) * 0.5)
            if not np.isfinite(gmean).all():
                return None
            vals, vecs = np.linalg.eigh((gmean + gmean.T) * 0.5)
    except np.linalg.LinAlgError:
        return None
    if not (np.isfinite(vals).all() and (vals > 0).all() and np.isfinite(vecs).all()):
        return None
    keep = (vals > eigval_cutoff) | (vals < 1.0 / eigval_cutoff)
    m = int(rank_multiple)
    if m > 1 and keep.sum() % m:
        want = min(dim, m * ((int(keep.sum()) + m - 1) // m))
        rest = np.flatnonzero(~keep)
        order = rest[np.argsort(-np.abs(np.log(vals[rest])), kind="stable")]
        keep[order[:want - int(keep.sum())]] = True
    if max_rank is not None and keep.sum() > max_rank:
        limit = int(max_rank) // max(m, 1) * max(m, 1) or int(max_rank)
        kept = np.flatnonzero(keep)
        order = kept[np.argsort(-np.abs(np.log(vals[kept])), kind="stable")]
        keep[order[limit:]] = False
    vals, vecs = vals[keep], vecs[:, keep]
    mu = dm + gm + vecs @ ((vals - 1.0) * (vecs.T @ gm))
    if not np.isfinite(mu).all():
        return None
    return sigma, mean, vals, np.ascontiguousarray(vecs.T), mu


def _stats_tensor(stats, n_rows, dev):
    """the rows' statistics as a [n_rows][sizeof(nm_draw_stats)] byte tensor on `dev` (a tensor is taken as it is)"""
    import torch
    from .sampler import STATS_DTYPE
    if isinstance(stats, torch.Tensor):
        st = stats.contiguous()
        if not st.is_cuda:
            st = st.to(dev)
    else:
        st = torch.from_numpy(np.ascontiguousarray(stats, dtype=STATS_DTYPE).view(np.uint8).reshape(-1).copy()).to(dev)
    if st.numel() * st.element_size() != n_rows * STATS_DTYPE.itemsize:
        raise ValueError("stats must hold one nm_draw_stats per row")
    return st


def pooled_scatter(rows, center, stats=None, stream=None):
    """S = sum over the kept rows of (x - center)(x - center)' for rows [..., dim] (nm_pooled_scatter, include/nuts_amd.h: the f64
    matrix cores, a stated summation order, no copy of the rows): returns (S [dim, dim], count).  stats: the rows' nm_draw_stats
    (a byte tensor or a STATS_DTYPE array, same row order) — only rows the pooled adaptation keeps then count; None: every row.
    float64 CUDA tensors are read where they lie, on `stream` (a torch.cuda.Stream; default torch's current one), and tensors are
    returned without waiting (count a one-element tensor); anything else goes through numpy and one upload, and arrays are returned."""
    import torch
    from . import _lib
    is_tensor = isinstance(rows, torch.Tensor)
    t = rows if is_tensor else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64))
    if t.dtype != torch.float64 or t.dim() < 1:
        raise ValueError("rows must be float64 [..., dim]")
    dim = int(t.shape[-1])
    n_rows = t.numel() // dim if dim else 0
    c = center if isinstance(center, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(center, dtype=np.float64))
    if c.dtype != torch.float64 or c.numel() != dim:
        raise ValueError("center must be float64 [dim]")
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        s = stream if stream is not None else cur
        if s != cur:
            s.wait_stream(cur)           # what the caller has queued for the inputs on torch's current stream comes first
        with torch.cuda.stream(s):       # every copy this call makes itself (contiguous, upload) is queued on the kernel's stream
            t = t.contiguous().to(dev)
            c = c.to(dev).contiguous()
            st = None if stats is None else _stats_tensor(stats, n_rows, dev)
            out = torch.empty((dim, dim), dtype=torch.float64, device=dev)
            cnt = torch.empty((1,), dtype=torch.float64, device=dev)
            L = _lib.load()
            _lib.check_status(L.nm_pooled_scatter(n_rows, dim, t.data_ptr() or None, c.data_ptr() or None, None if st is None else st.data_ptr(),
                                                  out.data_ptr() or None, cnt.data_ptr(), s.cuda_stream), L.nm_pooled_last_error)
            for keep in (t, c) + (() if st is None else (st,)):
                keep.record_stream(s)
    if is_tensor:
        return out, cnt
    s.synchronize()
    return out.cpu().numpy(), float(cnt.item())


def covariance_draws(draws, stats=None):
    """Posterior mean and covariance of a trace draws [n_draws, n_chains, dim], computed on the GPU where a CUDA tensor lies: the means
    are nm_pooled_partials', the scatter matrix about them nm_pooled_scatter's, cov = S / (count - 1).  Returns (mean [dim],
    cov [dim, dim], count) as numpy arrays and an int.  stats: the draws' nm_draw_stats — only the rows the pooled adaptation keeps."""
    import torch
    from . import _lib
    t = draws if isinstance(draws, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float64))
    if t.dtype != torch.float64 or t.dim() != 3:
        raise ValueError("draws must be float64 [n_draws, n_chains, dim]")
    t = t.contiguous()
    if not t.is_cuda:
        t = t.cuda()
    n_rows, dim = int(t.shape[0] * t.shape[1]), int(t.shape[2])
    with torch.cuda.device(t.device):
        s = torch.cuda.current_stream(t.device)
        st = None if stats is None else _stats_tensor(stats, n_rows, t.device)
        part = torch.empty((2, 1 + 2 * dim), dtype=torch.float64, device=t.device)
        L = _lib.load()
        # (nm_pooled_partials reduces draws AND gradients and takes no null for either: the draws stand in for the gradients, so the trace
        # is reduced a second time for a row of the result nobody reads — one more pass of three over the trace; a draws-only entry is not built)
        _lib.check_status(L.nm_pooled_partials(n_rows, dim, t.data_ptr() or None, t.data_ptr() or None, None if st is None else st.data_ptr(),
                                               part.data_ptr(), s.cuda_stream), L.nm_pooled_last_error)
        S, cnt = pooled_scatter(t, part[0, 1:1 + dim], stats=st, stream=s)
        s.synchronize()
    count = float(cnt.item())
    with np.errstate(all="ignore"):
        return part[0, 1:1 + dim].cpu().numpy(), S.cpu().numpy() / (count - 1.0), int(count)


def pooled_lowrank_warmup(batch, num_tune, windows=None, on_window=None):
    """Warm up `batch` (a ChainBatch created from LowRankNutsSettings(freeze_transform=True, num_tune=num_tune)) with ONE LOW-RANK
    transformation pooled over all its chains — the transformation the shared matrix-core draw kernels need (a full-precision normal,
    dim and rank multiples of 8).  Returns the list of (draw index, stds, mean, vals, vecs, mu_low_rank) updates.

    Same structure as pooled_warmup: every window records draws, gradients and statistics in device buffers; on a side stream, while
    the NEXT window's kernel runs, nm_pooled_partials gives count and means, two nm_pooled_scatter calls centred at those means give
    the scatter matrices of draws and gradients, the 2 (1 + D + D^2) doubles go to the host, lowrank_from_moments (gamma and
    eigval_cutoff of the batch's LowRankSettings; rank_multiple 8 where dim is a multiple of 8; at most the batch's lowrank_max_rank pairs)
    makes the estimate, and
    batch.set_transform applies it.  The transformation therefore lags the draws by ONE window, as in pooled_warmup.
    Single process: a driver over several ranks merges the ranks' triples with scatter_merge before the estimate."""
    import torch
    from .sampler import STATS_DTYPE
    dim, nc = batch.logp.dim, batch.n_chains
    mo = batch.settings.adapt_options.mass_matrix_options
    gamma, cutoff = float(mo.gamma), float(mo.eigval_cutoff)
    rank_multiple = 8 if dim % 8 == 0 else 1
    max_rank = batch.lowrank_max_rank()     # (dim unless the batch was created with a smaller lowrank_max_rank: set_transform refuses more)
    if windows is None:
        windows = window_schedule(num_tune)
    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(device=dev)
    updates, done, pending = [], 0, None

    def finish(p):
        payload, at = p
        side.synchronize()
        h = payload.cpu().numpy()
        one = 1 + dim + dim * dim
        x, g = h[:one], h[one:]
        est = lowrank_from_moments(float(x[0]), x[1:1 + dim], x[1 + dim:].reshape(dim, dim), g[1:1 + dim], g[1 + dim:].reshape(dim, dim),
                                   gamma, cutoff, rank_multiple=rank_multiple, max_rank=max_rank)
        if est is None:                 # fewer than three pooled draws, or a window that is not finite: keep the current transformation
            return
        batch.set_transform(*est)
        updates.append((at,) + est)
        if on_window:
            on_window(at, *est)

    for w in windows:
        pos = torch.empty((w, nc, dim), dtype=torch.float64, device=dev)
        grad = torch.empty((w, nc, dim), dtype=torch.float64, device=dev)
        # zero-filled statistics: a chain that has stopped writes no rows, and an all-zero row is not a draw the collector keeps
        stats = torch.zeros((w, nc, STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()       # (the fill runs on torch's stream, the engine on its own)
        batch.draw_device_ex(w, positions=pos.data_ptr(), stats=stats.data_ptr(), gradient=grad.data_ptr())     # the window's kernel
        if pending is not None:                # the previous window's moments were made beside this kernel; apply them now:
            finish(pending)                    # the pooled transformation lags the draws by ONE window (documented, deliberate)
        done += w
        with torch.cuda.stream(side):          # this window's moments, off the engine's stream
            for t in (pos, grad, stats):
                t.record_stream(side)
            part = _partials_device(pos, grad, stats, side)
            sx, _ = pooled_scatter(pos, part[0, 1:1 + dim], stats=stats, stream=side)
            sg, _ = pooled_scatter(grad, part[1, 1:1 + dim], stats=stats, stream=side)
            payload = torch.cat([part[0, :1 + dim], sx.reshape(-1), part[1, :1 + dim], sg.reshape(-1)])
        pending = (payload, done)
    if pending is not None:
        finish(pending)
    if done < num_tune:
        batch.draw_device(num_tune - done)     # the final window: step size only (reference adapt_strategy.rs:215-221)
    return updates
