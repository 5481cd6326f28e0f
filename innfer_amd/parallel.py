"""Multi-GPU chop_forward: tiles sharded over ranks, HR tiles collected on rank 0.

The reference is single-process; the only part of its hot path that shards is
Model.chop_forward's tile list (run.py:186-197: every tile's forward is independent,
the blend utils.py:436-443 is the single cross-tile step).  One process per GPU
(torch.distributed, backend "nccl" = RCCL over xGMI; "gloo" in the CPU tests and in the
one-GPU rehearsal):

  * every rank holds the (small) LR frame and cuts ITS contiguous range of the row-major
    tile list.  The split is even over TILES (798 tiles over 8 ranks -> 100,100,100,100,100,100,99,99:
    99.7 % balanced); SURVEY 8e's whole-tile-row blocks (21 rows -> 3,3,3,3,3,2,2,2: 87.5 %)
    stay available as shard='rows' -- they only matter for a design that blends per rank,
    and this one ships raw tiles so that the blend keeps the reference's accumulation order
    bit for bit;
  * each rank pushes its tiles through the network in batches;
  * ONE grouped exchange of the raw HR tiles: every rank r > 0 sends exactly its tiles (no
    padding) and rank 0 receives each share straight into its slot of the [n,C,P,P] tile
    buffer the blend kernel reads (RCCL: grouped ncclSend / ncclRecv, every peer pushes over
    its own xGMI link), then ONE blend kernel on rank 0.  The exchange is issued after the
    rank's last batch on purpose: the conv kernels are persistent, one workgroup per CU with the
    whole LDS, so an RCCL kernel spinning on a CU during the compute phase would stretch every
    layer by a whole tile round (the exchange is <= 5 % of a stage);
  * model chains: the blended intermediate is broadcast before the next stage.

No collective sits inside the per-tile compute.
"""
import math
import time

import torch
import torch.distributed as dist


def shard_tile_rows(n_rows, n_cols, world, rank):
    """Contiguous block of whole tile rows for `rank`: (first_tile, n_tiles).
    Rows are dealt as evenly as possible, earlier ranks take the remainder
    (43 rows over 8 ranks -> 6,6,6,5,5,5,5,5)."""
    base, rem = divmod(n_rows, world)
    rows = base + (1 if rank < rem else 0)
    first = rank * base + min(rank, rem)
    return first * n_cols, rows * n_cols


def shard_tiles(n_tiles, world, rank):
    """Contiguous range of the row-major tile list for `rank`: (first_tile, n_tiles); earlier
    ranks take the remainder (798 tiles over 8 ranks -> 100 x 6, 99 x 2)."""
    base, rem = divmod(n_tiles, world)
    return rank * base + min(rank, rem), base + (1 if rank < rem else 0)


MAX_TILE_BATCH = 272


def tile_batches(count, tile_batch=None, cap=None):
    """Sizes of the network launches for `count` tiles.  tile_batch=None: as few launches as fit `cap` tiles each (default MAX_TILE_BATCH), evenly
    sized (798 tiles -> 3 x 266).  A launch tiles its whole batch as ONE canvas (csrc/conv3x3.hip, conv3x3_pc<.., CV>) whose tile count is then
    rounded up to whole rounds of 256 workgroups: 64 tiles of 200^2 are 13.35 rounds (93 % useful), 266 are 54.8 (98 %).  The workspace of 272
    tiles of 200^2 is 64 GB of the 288 GB for a 4x RRDBNet in fp16 -- but 202 GiB at 8x and 770 GiB at 16x: callers that know their engine pass
    cap=engine_tile_cap(...), which sizes the launch from innfer_*_workspace_bytes and the free memory.  A number: fixed-size launches (the
    last one takes the remainder)."""
    if count <= 0:
        return []
    if tile_batch:
        return [min(tile_batch, count - i) for i in range(0, count, tile_batch)]
    cap = max(1, min(int(cap), MAX_TILE_BATCH)) if cap else MAX_TILE_BATCH
    nb = -(-count // cap)
    base, rem = divmod(count, nb)
    return [base + (1 if i < rem else 0) for i in range(nb)]


def free_device_bytes(device):
    """Bytes a new allocation can draw on: what the driver reports free plus the blocks torch's caching allocator holds without using them."""
    free, _ = torch.cuda.mem_get_info(device)
    return free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def engine_tile_cap(model_fn, ps, dtype, device, fraction=0.8, budget=None):
    """Largest tile batch (<= MAX_TILE_BATCH) whose engine workspace plus tile tensors fit `fraction` of the device's free memory (or `budget`
    bytes): model_fn.tile_batch_bytes(b, ps, dtype) when the callable has one (the nn.Module shells of innfer_amd do), MAX_TILE_BATCH otherwise.
    The engine's own workspace counts as free (it is re-used or replaced)."""
    cost = getattr(model_fn, 'tile_batch_bytes', None)
    if cost is None:
        return MAX_TILE_BATCH
    try:                                            # the nn.Module shells build their engine on the GPU the tiles are on (not on the current device)
        import inspect
        if 'device' in inspect.signature(cost).parameters and torch.device(device).type == 'cuda':
            import functools
            cost = functools.partial(cost, device=device)
    except (TypeError, ValueError):
        pass
    if budget is None:
        ws = getattr(model_fn, '_ws', None)
        budget = fraction * (free_device_bytes(device) + (ws.numel() if ws is not None else 0))
    if cost(MAX_TILE_BATCH, ps, dtype) <= budget:
        return MAX_TILE_BATCH
    lo, hi = 1, MAX_TILE_BATCH                      # cost is monotonic in the batch: largest b with cost(b) <= budget (at least 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if cost(mid, ps, dtype) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo


def run_tile_batches(model_fn, tiles, tile_batch=None, sink=None, pick=None, out=None):
    """tiles [n,C,ps,ps] through model_fn in batches (tile_batches with the engine's cap); an allocator out-of-memory halves the batch and goes
    on (the ladder VERDICT r2 asked for instead of a constant).  sink(i, y) receives batch i's result and nothing is returned; otherwise the results
    are returned concatenated.  pick: applied to model_fn's return value (PPON returns a tuple).
    out: a preallocated contiguous [n, C', P, P] tensor the results belong in (and the return value).  A model_fn that takes `out=` (the nn.Module
    shells: `_accepts_out`) writes every batch straight into its rows -- no per-batch result tensor, no copy, no concatenation;
    any other callable's results are copied there."""
    if out is not None and sink is not None:
        raise ValueError('run_tile_batches: give sink= or out=, not both (out= lands the results in the tile buffer; no sink calls are made)')
    n = tiles.shape[0]
    outs = []
    lands = out is not None and pick is None and bool(getattr(model_fn, '_accepts_out', False))
    ph, pw = tiles.shape[-2:]                       # rectangular tiles (Model.tile_forward): the cost of the square of the same area, an estimate -- the ladder below is the safety net
    cap = None if tile_batch else engine_tile_cap(model_fn, pw if ph == pw else math.isqrt(ph * pw - 1) + 1, tiles.dtype, tiles.device)
    i = 0
    while i < n:
        sizes = tile_batches(n - i, tile_batch, cap)
        b = sizes[0]
        try:
            y = model_fn(tiles[i:i + b], out=out[i:i + b]) if lands else model_fn(tiles[i:i + b])
        except torch.OutOfMemoryError:
            if b == 1:
                raise
            rel = getattr(model_fn, 'release_workspace', None)
            if rel is not None:
                rel()
            torch.cuda.empty_cache()
            tile_batch, cap = None, max(1, b // 2)
            continue
        if pick is not None:
            y = pick(y)
        if out is not None:
            if not lands:
                if y.shape[1:] != out.shape[1:] or y.dtype != out.dtype:
                    raise RuntimeError(f'run_tile_batches: model_fn returned {tuple(y.shape[1:])} {y.dtype}, the tile buffer is {tuple(out.shape[1:])} {out.dtype}')
                out[i:i + b].copy_(y)
        elif sink is not None:
            sink(i, y)
        else:
            outs.append(y)
        i += b
        del y
    if out is not None:
        return out
    if sink is not None:
        return None
    return torch.cat(outs, 0) if len(outs) != 1 else outs[0]


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


class CabiComm:
    """The C ABI's own RCCL communicator (include/innfer_amd.h: innfer_comm_init / innfer_gather_tiles / innfer_comm_broadcast) for the
    ranks of a torch.distributed group: rank 0 draws the ncclUniqueId, the group's store ships its 128 bytes, every rank joins on its
    current device.  What a C user of the library calls; ChopRunner(transport='cabi') routes its exchange through it."""

    def __init__(self, group=None):
        import ctypes as C
        from . import lib as L
        self._L, self.group = L, group
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        box = [None]
        if rank == 0:
            buf = (C.c_char * L.COMM_ID_BYTES)()
            L.check(L.lib.innfer_comm_unique_id(buf))
            box[0] = bytes(buf)
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        self.handle = C.c_void_p()
        L.check(L.lib.innfer_comm_init(C.byref(self.handle), box[0], rank, world))

    def gather_tiles(self, t, n_tiles):
        """t: rank 0 the whole [n_tiles, ...] buffer, other ranks their share (shard_tiles)."""
        tile_bytes = t[0].numel() * t.element_size() if t.shape[0] else 0
        if tile_bytes:
            self._L.check(self._L.lib.innfer_gather_tiles(self.handle, t.data_ptr(), tile_bytes, n_tiles,
                                                          torch.cuda.current_stream(t.device).cuda_stream))

    def broadcast(self, t, root=0):
        self._L.check(self._L.lib.innfer_comm_broadcast(self.handle, t.data_ptr(), t.numel() * t.element_size(), root,
                                                        torch.cuda.current_stream(t.device).cuda_stream))

    def __del__(self):
        h = getattr(self, 'handle', None)
        if h:
            try:
                self._L.lib.innfer_comm_destroy(h)
            except Exception:
                pass


class ChopRunner:
    """chop_forward (run.py:167-202) over `world` ranks.

    model_fn   : [n,C,ps,ps] -> [n,C',s*ps,s*ps] (an innfer_amd nn.Module on the GPU)
    tile_batch : tiles per network launch; None = evenly sized launches of at most MAX_TILE_BATCH tiles (tile_batches())
    extract_fn : (img, (ps,ps), [step,step], batch_first, tile_range) -> tiles, default HIP kernel
    recompose_fn: (tiles, H, W, step, scale) -> image, default HIP kernel
    plan_fn    : (H, W, patch, step) -> (ps, ys, xs), default the C ABI's innfer_chop_plan
    out_channels / out_dtype: shape and dtype of model_fn's output; every rank must agree on them BEFORE the
                 exchange (a rank may own no tile at all).  Defaults: model_fn.out_nc if it has one, else the
                 input's channel count; the input's dtype.
    shard      : 'tiles' (even split of the tile list) or 'rows' (whole tile rows)
    transport  : 'torch' (torch.distributed point-to-point ops: RCCL under the "nccl" backend, host staging under "gloo") or 'cabi' (the
                 library's own RCCL communicator, the entry points a C user binds: GPU tensors, shard='tiles' only)
    Returns the blended [1,C',sH,sW] tensor on rank 0 and None elsewhere
    (all ranks get it with broadcast_result=True, used between chained models).
    With profile=True every phase is bracketed by a device synchronise and `self.last` holds
    {tiles, compute_ms, exchange_ms, exchange_bytes, blend_ms, bcast_ms} of the call (never in a timed region).
    seamless   : must be None -- the seamless modes (Model.run_u8) are not built for the sharded chop: NotImplementedError.
    """

    def __init__(self, model_fn, scale, tile_batch=None, patch=200, step=0.5, group=None,
                 extract_fn=None, recompose_fn=None, plan_fn=None, out_channels=None, out_dtype=None,
                 shard='tiles', profile=False, transport='torch', seamless=None):
        if seamless is not None:
            raise NotImplementedError("ChopRunner: the seamless modes are built for Model.run_u8 on one GPU (the sharded chop works on tensors, whose "
                                      "tiles are cut from the image as it is); pad with utils.seamless_pad and crop with utils.seamless_crop around it")
        if shard not in ('tiles', 'rows'):
            raise ValueError("shard must be 'tiles' or 'rows'")
        if transport not in ('torch', 'cabi') or (transport == 'cabi' and shard != 'tiles'):
            raise ValueError("transport must be 'torch' or 'cabi' (the C ABI's partition is shard='tiles')")
        self.transport, self._cabi = transport, None
        self.model_fn, self.scale, self.tile_batch = model_fn, scale, tile_batch
        self.patch, self.step, self.group = patch, step, group
        self.out_channels, self.out_dtype, self.shard, self.profile = out_channels, out_dtype, shard, profile
        self.last = {}
        if extract_fn is None or recompose_fn is None or plan_fn is None:
            from . import lib as L
            from .utils import utils as U
            extract_fn = extract_fn or U.extract_patches_2d
            recompose_fn = recompose_fn or U.recompose_tensor
            plan_fn = plan_fn or L.chop_plan
        self.extract_fn, self.recompose_fn, self.plan_fn = extract_fn, recompose_fn, plan_fn

    def _world(self):
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.group), dist.get_rank(self.group)
        return 1, 0

    def _peer(self, r):
        return dist.get_global_rank(self.group, r) if self.group is not None else r

    def _share(self, n_rows, n_cols, world, rank):
        if self.shard == 'rows':
            return shard_tile_rows(n_rows, n_cols, world, rank)
        return shard_tiles(n_rows * n_cols, world, rank)

    def _staged(self, t):
        """gloo moves host memory only: the one-GPU rehearsal (all ranks on one device) stages through the host."""
        return t.is_cuda and dist.get_backend(self.group) == 'gloo'

    def __call__(self, data, broadcast_result=False):
        world, rank = self._world()
        prof = self.profile
        _, C, H, W = data.shape
        ps, ys, xs = self.plan_fn(H, W, self.patch, self.step)
        n_rows, n_cols = len(ys), len(xs)
        n = n_rows * n_cols
        first, count = self._share(n_rows, n_cols, world, rank)
        P = ps * self.scale
        out_c = self.out_channels or getattr(self.model_fn, 'out_nc', None) or C
        dtype = self.out_dtype or data.dtype
        if prof:
            _sync(data)
            t0 = time.perf_counter()
        # rank 0 owns the whole [n,C',P,P] buffer the blend reads, the others only their share; batches land in place
        hr = torch.empty((n if rank == 0 else count, out_c, P, P), dtype=dtype, device=data.device)
        if count:
            tiles = self.extract_fn(data, (ps, ps), [self.step, self.step], batch_first=True,
                                    tile_range=(first, count)).squeeze(0)
            base = first if rank == 0 else 0
            with torch.no_grad():               # batches land in their rows of the tile buffer (engines: written there by the last conv, no copy)
                try:
                    run_tile_batches(self.model_fn, tiles, self.tile_batch, out=hr[base:base + count])
                except (RuntimeError, ValueError) as e:
                    if 'tile buffer' in str(e) or 'out= must be' in str(e):
                        raise RuntimeError(f'ChopRunner: every rank was told model_fn returns {tuple(hr.shape[1:])} {hr.dtype} (set out_channels / out_dtype): {e}') from None
                    raise
            del tiles
        if prof:
            _sync(data)
            t1 = time.perf_counter()
        xbytes = 0
        if world > 1 and self.transport == 'cabi':
            if self._cabi is None:
                self._cabi = CabiComm(self.group)
            self._cabi.gather_tiles(hr, n)
            tb = out_c * P * P * hr.element_size()
            xbytes = (n - count if rank == 0 else count) * tb
        elif world > 1:
            # ---- grouped point-to-point exchange: real tiles only, received in place ----
            ops, stage = [], []
            if rank == 0:
                for r in range(1, world):
                    f, c = self._share(n_rows, n_cols, world, r)
                    if not c:
                        continue
                    dst = hr[f:f + c]
                    xbytes += dst.numel() * dst.element_size()
                    if self._staged(dst):
                        buf = torch.empty(dst.shape, dtype=dst.dtype, device='cpu')
                        stage.append((dst, buf))
                        dst = buf
                    ops.append(dist.P2POp(dist.irecv, dst, self._peer(r), self.group))
            elif count:
                src = hr.cpu() if self._staged(hr) else hr
                xbytes = hr.numel() * hr.element_size()
                ops.append(dist.P2POp(dist.isend, src, self._peer(0), self.group))
            if ops:
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
            for dst, buf in stage:
                dst.copy_(buf)
        if prof:
            _sync(data)
            t2 = time.perf_counter()
        result = None
        if rank == 0:
            result = self.recompose_fn(hr, H, W, step=self.step, scale=self.scale)
        del hr
        if prof:
            _sync(data)
            t3 = time.perf_counter()
        if broadcast_result and world > 1:
            if rank != 0:
                result = torch.empty((1, out_c, H * self.scale, W * self.scale), dtype=dtype, device=data.device)
            if self.transport == 'cabi':
                self._cabi.broadcast(result, 0)
            elif self._staged(result):
                buf = result.cpu() if rank == 0 else torch.empty(result.shape, dtype=dtype, device='cpu')
                dist.broadcast(buf, src=self._peer(0), group=self.group)
                if rank != 0:
                    result.copy_(buf)
            else:
                dist.broadcast(result, src=self._peer(0), group=self.group)
        if prof:
            _sync(data)
            t4 = time.perf_counter()
            self.last = {'tiles': count, 'tiles_total': n, 'compute_ms': (t1 - t0) * 1e3, 'exchange_ms': (t2 - t1) * 1e3,
                         'exchange_bytes': xbytes, 'blend_ms': (t3 - t2) * 1e3, 'bcast_ms': (t4 - t3) * 1e3}
        return result


def run_chain(runners, data, seamless=None):
    """Model chain `a+b` (run.py:424-426): every stage is tile-sharded; the blended
    intermediate is broadcast so each rank can cut its own next-stage tiles.  seamless must be None (see ChopRunner)."""
    if seamless is not None:
        raise NotImplementedError("run_chain: the seamless modes are not built for the sharded chop; pad and crop around it (utils.seamless_pad / seamless_crop)")
    x = data
    for i, r in enumerate(runners):
        x = r(x, broadcast_result=(i + 1 < len(runners)))
    return x
