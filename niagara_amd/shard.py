"""Sharding of the visibility pass across the GPUs of one node: one process per GPU, contiguous command
ranges per rank, no exchange of meshlet data; the only collective is one all-reduce (sum) of the visible counts per
phase — RCCL over xGMI when the process group is "nccl", gloo in the CPU tests.

A whole frame is sharded by contiguous ranges of DRAWS (pipeline.ShardedVisibilityPipeline): draw_ranges picks the
ranges, composite_depth is the one exchange the closed loop adds (the element-wise maximum of the ranks' depth targets;
composite_visibility the same for the stable-ID visibility buffer), and the
stitch_* helpers put the ranks' outputs back together into the unsharded frame's, bit for bit.

The reference has no multi-GPU path (one VkPhysicalDevice, src/device.cpp:190-248); this is the new part.
"""
import numpy as np

from . import host


def command_range(command_count, rank, world):
    """contiguous [begin, end) of task commands owned by `rank` (nv_shard_range)"""
    return host.shard_range(command_count, rank, world)


def local_commands(commands, begin, end):
    """the rank's slice, padded with zeroed dummy commands to a multiple of 64 like tasksubmit does"""
    n = end - begin
    out = np.zeros((n + 63) // 64 * 64, dtype=commands.dtype)
    out[:n] = commands[begin:end]
    return out, n


def to_global_ids(local_ids, command_base):
    """clusterIndices entries are commandId (24 bits) | lane << 24 (clustercull.comp.glsl:138); rebase the rank-local
    command id by the first command the rank owns"""
    local_ids = np.asarray(local_ids, dtype=np.uint32)
    pad = local_ids == np.uint32(0xffffffff)  # clustersubmit's padding entries (clustersubmit.comp.glsl:41-44) stay ~0
    cmd = (local_ids & np.uint32(0xffffff)).astype(np.uint64) + np.uint64(command_base)
    if cmd.size and int(cmd[~pad].max(initial=0)) >= 1 << 24:
        raise ValueError("global command id does not fit the 24-bit field of a cluster index")
    out = cmd.astype(np.uint32) | (local_ids & np.uint32(0xff000000))
    out[pad] = np.uint32(0xffffffff)
    return out


def draw_weights(draws, meshes):
    """per draw: the meshlet count of its mesh's largest LOD — what the draw costs the cluster passes at most"""
    if not len(draws) or not len(meshes):
        return np.zeros(len(draws), np.int64)
    counts = meshes["lods"]["meshletCount"].astype(np.int64)
    valid = np.arange(counts.shape[1])[None, :] < meshes["lodCount"][:, None]
    per_mesh = np.where(valid, counts, 0).max(axis=1)
    return per_mesh[np.minimum(draws["meshIndex"].astype(np.int64), len(meshes) - 1)]


def draw_ranges(draws, meshes, world, weight="draws"):
    """[(begin, end)] * world: contiguous ranges of draws in rank order that cover [0, len(draws)).

    weight="draws": equal counts (nv_shard_range).  weight="meshlets": boundary k is the draw whose prefix of draw_weights is
    nearest to k / world of the total, so every boundary is within half the heaviest draw's weight of the ideal split; equal
    draw counts balance nothing when the meshes differ.  With at least `world` draws no range is empty (a boundary that would
    coincide with its neighbour moves by one draw: an idle rank is worse than an uneven one); with fewer, some ranges are."""
    n, world = len(draws), int(world)
    if world < 1:
        raise ValueError("world must be >= 1")
    if weight == "draws":
        return [tuple(host.shard_range(n, r, world)) for r in range(world)]
    if weight != "meshlets":
        raise ValueError("weight must be 'draws' or 'meshlets'")
    prefix = np.concatenate([[0], np.cumsum(draw_weights(draws, meshes))]).astype(np.int64)
    total = int(prefix[-1])
    if total == 0:
        return [tuple(host.shard_range(n, r, world)) for r in range(world)]
    bounds = [0]
    for k in range(1, world):
        i = int(np.searchsorted(prefix * world, total * k))  # first prefix >= the ideal total * k / world (exact in integers)
        if i > 0 and total * k - int(prefix[i - 1]) * world <= int(prefix[i]) * world - total * k:
            i -= 1
        if n >= world:
            i = min(max(i, bounds[-1] + 1), n - (world - k))
        bounds.append(max(i, bounds[-1]))
    bounds.append(n)
    return [(bounds[r], bounds[r + 1]) for r in range(world)]


def composite_depth(depth, group=None):
    """The depth composite of a sharded frame, in place on every rank: depth = element-wise maximum over the ranks of `group`
    (a torch.distributed process group, or True for the default one).  It is one all_reduce(MAX) of the target viewed as int32: for
    the values the rasterisers write (reverse-Z in [0, 1], never negative, never NaN) the signed maximum of the bits is the maximum
    of the floats, exact and independent of the order of the ranks.  Runs on the caller's current stream (nccl / RCCL: on device
    memory; gloo stages through the host), and returns when the collective is enqueued (nccl) or done (gloo).  group=None: nothing
    to exchange, a no-op.  Shards of one process fold their targets with nv_depth_merge instead (Context.depth_merge)."""
    if group is None:
        return depth
    import torch
    import torch.distributed as dist
    dist.all_reduce(depth.view(torch.int32), op=dist.ReduceOp.MAX, group=None if group is True else group)
    return depth


def composite_visibility(visibility, group=None):
    """The composite of a sharded frame's stable-form visibility targets (NV_OPT_RASTER_VISIBILITY_ID 1), in place on every rank: the
    element-wise UNSIGNED 64-bit maximum over the ranks of `group`, as one all_reduce(MAX).  Neither backend reduces unsigned 64-bit
    integers, and bit 63 of a word can be set (bits(1.0) << 34 = 0x3F800000 << 34), so the signed maximum of the int64 view would order such
    words below all others: the sign bit is flipped before and after (x ^ 1 << 63), which maps unsigned order onto signed order — an
    order-preserving bijection, so max commutes with it.  `visibility` is an int64 (or uint64-viewed) tensor; group=None is a no-op.
    Shards of one process fold their targets with nv_visibility_merge instead (Context.visibility_merge)."""
    if group is None:
        return visibility
    import torch
    import torch.distributed as dist
    v = visibility.view(torch.int64)
    sign = torch.tensor(-(1 << 63), dtype=torch.int64, device=v.device)
    v.bitwise_xor_(sign)
    dist.all_reduce(v, op=dist.ReduceOp.MAX, group=None if group is True else group)
    v.bitwise_xor_(sign)
    return visibility


def to_global_draw_ids(commands, draw_base):
    """a copy of a rank's MeshTaskCommands or MeshDrawCommands with the rank-local drawId rebased by the first draw the rank owns"""
    out = np.array(commands, copy=True)
    if len(out) and int(out["drawId"].max()) + int(draw_base) >= 1 << 32:
        raise ValueError("global draw id does not fit 32 bits")
    out["drawId"] += np.uint32(draw_base)
    return out


def stitch_commands(parts, ranges):
    """parts[r]: the commands rank r appended (count4[0] of them, no tasksubmit padding); ranges: draw_ranges.  Returns the unsharded
    pass's command list: append order is ascending draw index and the ranges are contiguous, so it is the concatenation in rank order"""
    return np.concatenate([to_global_draw_ids(p, b) for p, (b, _) in zip(parts, ranges)])


def stitch_cluster_ids(parts, command_counts):
    """parts[r]: rank r's cluster indices (ccb[0] of them, or with clustersubmit's ~0 padding, which is dropped); command_counts[r]: the
    commands rank r appended (dccb[0]).  The command id of rank r's entries is rebased by the commands of the ranks before it"""
    out, base = [], 0
    for ids, n in zip(parts, command_counts):
        ids = np.asarray(ids, dtype=np.uint32)
        out.append(to_global_ids(ids[ids != np.uint32(0xffffffff)], base))
        base += int(n)
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def stitch_visibility(dvb_parts, mvb_parts):
    """(dvb, mvb) of the unsharded frame: dvb_parts[r] is rank r's drawVisibility over ITS draws, concatenated; mvb_parts[r] is rank r's
    full-size meshletVisibility, of which it only ever set bits of its own draws (meshletVisibilityOffset is the global prefix): OR"""
    mvb = np.zeros_like(np.asarray(mvb_parts[0], dtype=np.uint32))
    for m in mvb_parts:
        mvb |= np.asarray(m, dtype=np.uint32)
    return np.concatenate([np.asarray(d, dtype=np.uint32) for d in dvb_parts]), mvb


class CountsReducer:
    """The passes' counts {0, task commands, visible meshlets} summed over the ranks — the one collective of the sharded
    path.  Nothing on the data path waits for it, so it is kept off the critical path twice over:
    the scatter launch writes the payload itself (nv_set_counts_sink: no extra launch per pass) into row i % B of a
    [B, 3] int64 block, and the block is reduced B passes at a time with ONE asynchronous all-reduce on the collective's
    own stream, waited for only when the block comes round again (two blocks alternate).  B = 1: one collective per pass.

        red = CountsReducer(ctx, device, batch)
        for i in range(steps): red.before_pass(i); ctx.clustercull(...); red.after_pass(i)
        red.drain(steps); total = red.last(steps)          # int64[3], summed over the ranks (world size 1: the pass's own counts)

    After a block's in-place all-reduce its rows hold SUMS; a pass overwrites its own row before the block is reduced again, and
    drain() zeroes the rows a partial last batch did not write before it reduces that block.  So: call drain(n) before last(n),
    and do not read a block between before_pass and drain — rows not yet rewritten still hold the previous use's sums.
    """

    def __init__(self, ctx, device, batch=8, stream=None, force_collective=False):
        import contextlib
        import torch
        import torch.distributed as dist
        self.ctx, self.dist, self.B = ctx, dist, max(1, int(batch))
        # the stream the context's passes are launched on (None: the current one): the collective is ordered behind it and
        # waits are issued on it
        self._on = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # force_collective (bench.py --force-sharded): issue the all-reduces also in a process group of ONE rank — the sharded path
        # (asynchronous batched all-reduce on device tensors, its stream ordering, the waits) executed over RCCL on a one-GPU box
        self.collective = self.world > 1 or (bool(force_collective) and dist.is_available() and dist.is_initialized())
        self.blocks = [torch.zeros((self.B, 3), dtype=torch.int64, device=device) for _ in range(2)]
        self.pending = [None, None]
        # the rows' addresses, marshalled once: before_pass runs once per pass, and a pass is ~30 us
        import ctypes
        from ._lib import lib
        self._sink = lib.nv_set_counts_sink
        self._rows = [[ctypes.c_void_p(self.blocks[k][r].data_ptr()) for r in range(self.B)] for k in range(2)]

    def before_pass(self, i):
        blk, row = (i // self.B) % 2, i % self.B
        if not self.collective:  # nothing to sum: the scatter launch still leaves the pass's counts in its row, so last() holds for any world size
            self._sink(self.ctx.h, self._rows[blk][row])
            return
        if row == 0:
            with self._on():
                if self.pending[blk] is not None:
                    self.pending[blk].wait()  # the block's previous reduction (issued 2 B passes ago)
                    self.pending[blk] = None
        self._sink(self.ctx.h, self._rows[blk][row])

    def after_pass(self, i):
        if self.collective and i % self.B == self.B - 1:
            blk = (i // self.B) % 2
            with self._on():
                self.pending[blk] = self.dist.all_reduce(self.blocks[blk], async_op=True)

    def drain(self, n_steps):
        """reduces the rows of a batch the loop left unfinished, then waits for everything in flight"""
        if not self.collective:
            return
        with self._on():
            if n_steps % self.B:
                blk = (n_steps // self.B) % 2
                self.blocks[blk][n_steps % self.B:].zero_()  # rows this partial batch did not write still hold an earlier use's sums
                self.pending[blk] = self.dist.all_reduce(self.blocks[blk], async_op=True)
            for k in range(2):
                if self.pending[k] is not None:
                    self.pending[k].wait()
                    self.pending[k] = None

    def last(self, n_steps):
        """the summed counts of pass n_steps - 1 (after drain)"""
        return self.blocks[((n_steps - 1) // self.B) % 2][(n_steps - 1) % self.B].clone()


def allreduce_counts(counts):
    """counts: int64 tensor {commands, task groups, visible meshlets}; summed in place over all ranks"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
    return counts
