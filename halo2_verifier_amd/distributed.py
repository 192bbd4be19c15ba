"""Sharded verification of one batch across the GPUs of a node (one process per GPU).

The reference has no communication layer.  Proofs are independent until the final pairing, so the batch is cut
into contiguous shards; every rank runs the whole per-proof pipeline and its two pooled MSMs, and the only exchange is an
all-gather of one 1312-byte record per rank and group (the two accumulators in the six pieces the launch leaves them in, 108 bytes
each, + the shard's failed-proof count) — RCCL has no user-defined reduction, and a group addition is not a numeric sum — followed
by a piece-wise fold and ONE pairing over the pieces (DualMSM::add_msm + check, poly/kzg/msm.rs:173-203).

Multipliers: proof i of the whole batch is scaled by the product of the Fr::random draws of all later proofs
(kzg/strategy.rs:129, msm.rs:173-176), indexed globally, so the result does not depend on the number of ranks: a rank uploads the
draws from its first proof to the END of the batch (its "tail").

Entry points
  verify_batch_sharded(ctx, proofs, instances, rand=None, group=None, seed=None)
      N x verify_proof on ONE AccumulatorStrategy + finalize(), the proofs sharded over the ranks of a torch.distributed group.
      Every rank passes the whole batch and gets the same (ok, statuses, left_xy, right_xy).  With seed (True: common_seed, one
      32-byte broadcast; bytes: given) the draws are draws.expand(seed, 0, n) and every rank expands only its own tail
      (seeded_tail, seeded_tail_tensor): no n x 32-byte broadcast.
  verify_batch_sharded_local(ctx, proofs, instances, rand, world)
      the same computation with the `world` shards run one after the other on ONE GPU (no process group): sharding invariance
      at full size on a single device, and hosts with one GPU.
  verify_batch_sharded_identify / verify_batch_sharded_local_identify
      the same two with the failing proofs named: statuses[i] is what SingleStrategy reports for proof i.  Every rank searches its
      own shard only (ShardedBatch.identify), and nothing but the existing status gather crosses ranks.
  ShardedBatch
      the staged form both are built on (and bench.py pipelines): upload the shard once, launch() = shard pipeline -> export ->
      all-gather -> fold -> one pairing, asynchronous on the batch's stream; finish() fetches the verdict.
  ShardedAccumulator(ctx, group=None, device=None)
      the streaming form: every rank owns a resident Accumulator and feeds it its own proofs as they arrive, with no collective per
      leg; finalize() all-gathers the 152-byte states, takes one fresh draw per rank and merges them under ONE pairing
      (Accumulator.merge_states), check_ranks() names the ranks whose own accumulator fails.
  merge_accumulators_local(ctx, accumulators, draws)
      the same merge over accumulators of one GPU (several feeder threads; tests).
Neither the sharded batch nor the sharded accumulator has run over RCCL with more than one rank: the multi-rank tests run over gloo.
"""
import contextlib
import ctypes
import hashlib
import os

from . import _lib

_FR_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def shard_bounds(total: int, world_size: int, rank: int):
    """Contiguous shard [lo, hi) of `total` proofs for `rank`."""
    base, rem = divmod(total, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


# include/h2v.h H2V_ACC_RECORD_BYTES: [u32 failed proofs of the shard][u32 parts][u32 shift][u32 0] + 2 x 6 Jacobian G1 pieces
# (3 coordinates x 9 limbs x 4 B, the library's Montgomery limb layout).  The count travels with the points so that every rank
# clears the verdict when ANY shard rejected a proof (a failed proof contributes nothing to its shard's accumulators).
ACC_BYTES = 16 + 2 * 6 * 108


def gather_accumulators(local_acc, world_size, group=None):
    """all_gather of the per-rank accumulator bytes (torch uint8 tensor of groups * ACC_BYTES, as Batch.export_accumulators
    writes them) -> tensor [world_size * groups * ACC_BYTES], the layout Batch.fold_check_enqueue folds group by group.
    Works with the nccl (= RCCL) backend on GPU tensors and with gloo on CPU tensors (tests)."""
    import torch
    import torch.distributed as dist
    out = torch.empty(world_size * local_acc.numel(), dtype=torch.uint8, device=local_acc.device)
    if world_size == 1:
        out.copy_(local_acc)
        return out
    dist.all_gather_into_tensor(out, local_acc, group=group)
    return out


def tail_for_shard(rand_all: bytes, lo: int):
    """The draws this shard needs: those of proofs [lo, total)."""
    return rand_all[32 * lo:]


def draw_scalars(n: int) -> bytes:
    """n x Fr::random(OsRng) as AccumulatorStrategy::process draws them (kzg/strategy.rs:129): 64 OS-random bytes reduced mod r,
    32 little-endian canonical bytes each."""
    try:   # the library's own generator (h2v_random_scalars: what rand32 = NULL draws inside the one-shot entry points)
        lib = _lib.load_library()
    except (_lib.H2VError, OSError, AttributeError):   # library missing or stale (orchestration tests without the product): the same distribution from os.urandom
        return b"".join((int.from_bytes(os.urandom(64), "little") % _FR_MODULUS).to_bytes(32, "little") for _ in range(n))
    buf = ctypes.create_string_buffer(max(32 * n, 1))
    _lib.check(lib.h2v_random_scalars(buf, n))   # (a failing generator is an error, never replaced by other draws)
    return buf.raw[: 32 * n]


def _scalar_bytes(rand) -> bytes:
    out = bytearray()
    for r in rand:
        if isinstance(r, (bytes, bytearray, memoryview)):
            if len(r) != 32:
                raise ValueError("a draw given as bytes must be exactly 32 bytes")
            out += bytes(r)
        else:
            r = int(r)
            if r < 0 or r >> 256:
                raise ValueError("a draw given as an integer must be in [0, 2^256)")
            out += r.to_bytes(32, "little")
    return bytes(out)


def _group_info(group):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0, 1, None
    return dist.get_rank(group), dist.get_world_size(group), dist.get_backend(group)


def common_draws(n: int, rand, group=None, device=None) -> bytes:
    """The ONE stream of Fr::random draws every rank of a sharded batch must use: `rand` (n ints / 32-byte strings, the same on
    every rank) or, when None, drawn by rank 0 from the OS and broadcast.  -> n * 32 bytes."""
    rank, world, backend = _group_info(group)
    if rand is not None:
        if len(rand) != n:
            raise ValueError(f"rand must hold one scalar per proof ({n}), got {len(rand)}")
        return _scalar_bytes(rand)
    if world == 1:
        return draw_scalars(n)
    import torch
    import torch.distributed as dist
    dev = device if (backend == "nccl" and device is not None) else "cpu"
    buf = torch.zeros(max(32 * n, 1), dtype=torch.uint8, device=dev)
    if rank == 0 and n:
        buf[: 32 * n] = torch.frombuffer(bytearray(draw_scalars(n)), dtype=torch.uint8).to(dev)
    dist.broadcast(buf, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return bytes(buf[: 32 * n].cpu().numpy().tobytes())


def common_draws_tensor(n: int, rand, group=None, device=None):
    """common_draws as a uint8 tensor [n, 32] on `device`, for ShardedBatch.upload_tensors (a shard's tail is the rows from its first
    proof on).  Under nccl with `rand` None the draws rank 0 made are broadcast on the device and stay there: no copy back to the host.
    In every other case (given draws, a world of one, gloo) the bytes of common_draws are copied to the device."""
    import torch
    rank, world, backend = _group_info(group)
    if rand is not None or world == 1 or backend != "nccl" or device is None:
        flat = common_draws(n, rand, group, device)
        return torch.frombuffer(bytearray(flat) if n else bytearray(32), dtype=torch.uint8)[: 32 * n].reshape(n, 32).to(device if device is not None else "cpu")
    import torch.distributed as dist
    buf = torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=device)
    if rank == 0 and n:
        buf[:n] = torch.frombuffer(bytearray(draw_scalars(n)), dtype=torch.uint8).reshape(n, 32).to(device)
    dist.broadcast(buf, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return buf[:n]


def common_seed(group=None, device=None) -> bytes:
    """The ONE 32-byte seed every rank of a sharded batch expands its draws from (draws.expand): rank 0 takes it from the OS and
    broadcasts it — one 32-byte broadcast, whatever the size of the batch."""
    from . import draws
    rank, world, backend = _group_info(group)
    if world == 1:
        return draws.new_seed()
    import torch
    import torch.distributed as dist
    dev = device if (backend == "nccl" and device is not None) else "cpu"
    buf = torch.zeros(32, dtype=torch.uint8, device=dev)
    if rank == 0:
        buf[:] = torch.frombuffer(bytearray(draws.new_seed()), dtype=torch.uint8).to(dev)
    dist.broadcast(buf, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return bytes(buf.cpu().numpy().tobytes())


def _resolve_seed(seed, group=None, device=None) -> bytes:
    """seed=True: common_seed; bytes: a given seed, the same on every rank"""
    return common_seed(group, device) if seed is True else bytes(seed)


def seeded_tail(seed: bytes, lo: int, total: int, groups: int = 1) -> bytes:
    """The draws a shard needs, from a seed, on the host: the whole stream is draws.expand(seed, 0, groups * total), group g owns
    indices [g * total, (g + 1) * total), and the shard that starts at proof `lo` of every group takes [g * total + lo, (g + 1) *
    total) of each, group-major."""
    from . import draws
    return b"".join(draws.expand(seed, g * total + lo, total - lo) for g in range(groups))


def seeded_tail_tensor(seed: bytes, lo: int, total: int, groups: int = 1, device=None, stream=None):
    """seeded_tail in device memory -> uint8 tensor [groups * (total - lo), 32] on `device`, a kernel per group on `stream`
    (draws.expand_into's rules; None = torch's current stream).  No draw bytes cross to the device and nothing waits."""
    import torch
    from . import draws
    if not 0 <= lo <= total or groups < 1:
        raise ValueError(f"a shard starts inside its batch: lo = {lo}, total = {total}, groups = {groups}")
    per = total - lo
    out = torch.empty((groups * per, 32), dtype=torch.uint8, device=device)
    for g in range(groups):
        if per:
            draws.expand_into(seed, g * total + lo, out[g * per:(g + 1) * per], stream)
    return out


class ShardedBatch:
    """One rank's share of a sharded batch (or of `groups` independent sharded batches that travel in one launch), resident on
    its GPU.  launch() enqueues, on the batch's stream and without host synchronisation: the shard's pipeline up to its two
    accumulators -> their records -> all-gather over the group -> fold -> ONE pairing per group; finish() returns what every rank
    agrees on.  With a world of one the launch simply ends in its own pairing.

    stream: a torch.cuda.Stream (or a raw HIP stream handle) the batch runs on — collectives are issued under the same stream, so MSM,
    all-gather and pairing are ordered without host synchronisation; None: a stream of the batch's own.
    batch_factory(ctx, max_proofs, max_instance_values, stream, groups) builds the object that runs a shard; the default is the
    HIP batch (verifier.Batch) — there is no CPU path in the product (the non-GPU test suite injects a stand-in to exercise the
    orchestration over gloo)."""

    def __init__(self, ctx, max_proofs: int, max_instance_values: int = 0, groups: int = 1, group=None, stream=None, device=None,
                 batch_factory=None, world_size=None, always_exchange=False):
        import torch
        self.rank, self.world, self.backend = _group_info(group)
        if world_size is not None:        # sequential simulation of `world_size` ranks (verify_batch_sharded_local): no process group
            self.world = world_size
        self.group, self.groups = group, groups
        self.always_exchange = always_exchange   # a world of one still runs export -> gather -> fold (what sharding costs besides the collective)
        if batch_factory is None:
            from .verifier import Batch
            batch_factory = lambda c, n, mi, st, g: Batch(c, n, mi, stream=st, groups=g)
            if device is None:
                device = f"cuda:{ctx.device}"
        self.device = torch.device(device if device is not None else "cpu")
        self._torch_stream = None
        if stream is not None and hasattr(stream, "cuda_stream"):   # a torch.cuda.Stream: collectives are issued under it as it is
            self._torch_stream = stream
            stream = stream.cuda_stream
        if stream is None and self.device.type == "cuda" and self.world > 1 and world_size is None:
            # the collective must be ordered with the batch's kernels: run both on one torch stream
            self._torch_stream = torch.cuda.Stream(device=self.device)
            stream = self._torch_stream.cuda_stream
        self._stream_handle = stream
        self.batch = batch_factory(ctx, max(max_proofs, 1), max_instance_values, stream, groups)
        self.records = torch.zeros(ACC_BYTES * groups, dtype=torch.uint8, device=self.device)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)   # (allocated and zeroed on torch's current stream, written on the batch's)
        self.gathered = None
        self._exchanged = False     # the last launch exported its records (and a fold may have replaced the batch's own accumulators)
        self._finished = None       # what the last finish() returned

    def close(self):
        if self.batch is not None:
            self.batch.close()
            self.batch = None

    def upload(self, proofs_flat: bytes, proof_len: int, instances_flat: bytes, col_lens, rand_tail: bytes):
        """This rank's shard (of every group: group-major) and, per group, the draws from its first proof to the end of the
        group's whole batch."""
        self.batch.upload(proofs_flat, proof_len, instances_flat, col_lens, rand_tail)

    def upload_tensors(self, proofs, instances, col_lens, rand_tail=None, seed=None, lo=None, total=None):
        """upload() for a shard that is already in device memory (Batch.upload_tensors): uint8 tensors on the batch's device, proofs
        [n, >= proof length], instances [n, sum(col_lens) * 32] or None, rand_tail [n_tail, 32] — common_draws_tensor's rows from the
        shard's first proof on.  Device work only, ordered behind the tensors' current stream; no host wait.
        seed (instead of rand_tail) with lo and total: the shard starts at proof `lo` of a batch of `total` proofs per group, and its
        tail is seeded_tail_tensor(seed, lo, total, groups), expanded on the batch's stream: the rank receives 32 bytes, not the draws."""
        if seed is None:
            if lo is not None or total is not None:
                raise ValueError("lo and total go with seed")
            self.batch.upload_tensors(proofs, instances, col_lens, rand_tail)
            return
        if rand_tail is not None:
            raise ValueError("give the draws (rand_tail) or the seed they come from, not both")
        if lo is None or total is None:
            raise ValueError("a seeded shard needs its place in the batch: lo and total")
        tail = seeded_tail_tensor(seed, lo, total, self.groups, proofs.device, self.batch.stream)
        try:
            self.batch.upload_tensors(proofs, instances, col_lens, tail)
        finally:
            self.batch.hold_tail(tail)   # (no caller holds this tensor: the batch does, until its stream has read it)

    def set_hints(self, y32):
        """Point hints for this rank's upload (Batch.set_hints): the rows of the rank's own proofs, n * n_points * 32 bytes, or None.
        Hints are a rank's own business: they change its launch's time and nothing that is exchanged."""
        self.batch.set_hints(y32)

    def set_hint_rows(self, rows):
        """The same from one row or None per proof of this rank's upload (Batch.set_hint_rows)."""
        self.batch.set_hint_rows(rows)

    def launch_shard(self):
        """Shard pipeline without a pairing + export of the accumulator records -> the local record tensor (stream-ordered)."""
        self.batch.launch(with_pairing=False)
        self.batch.export_accumulators(self.records.data_ptr())
        self._exchanged = True
        return self.records

    def fold(self, gathered, n_records: int):
        """Fold `n_records` gathered record sets ([rank][group]) and enqueue the one pairing per group."""
        self.gathered = gathered      # kept alive until finish()
        self.batch.fold_check_enqueue(gathered.data_ptr(), n_records)

    def upload_launch(self, proofs_flat: bytes, proof_len: int, instances_flat: bytes, col_lens, rand_tail: bytes):
        """upload() + launch() with the host -> device copy of the shard hidden behind its point decompression
        (h2v_batch_upload_launch): for shards that arrive from the host for every batch."""
        if self.world == 1 and not self.always_exchange:
            self.batch.upload_launch(proofs_flat, proof_len, instances_flat, col_lens, rand_tail, with_pairing=True)
            self._exchanged = False
            return
        with self._on_stream():
            self.batch.upload_launch(proofs_flat, proof_len, instances_flat, col_lens, rand_tail, with_pairing=False)
            self.batch.export_accumulators(self.records.data_ptr())
            self._exchanged = True
            self.fold(gather_accumulators(self.records, self.world, self.group), self.world)

    def launch(self):
        if self.world == 1 and not self.always_exchange:
            self.batch.launch(with_pairing=True)
            self._exchanged = False
            return
        with self._on_stream():
            local = self.launch_shard()
            self.fold(gather_accumulators(local, self.world, self.group), self.world)

    def _on_stream(self):
        """The context an exchanging launch runs under: the batch's stream as torch's current one, so that the collective is ordered with
        the batch's kernels (nothing to enter without a GPU stream)"""
        import torch
        if self.device.type == "cuda" and self._stream_handle is not None:
            return torch.cuda.stream(self._external_stream())
        return contextlib.nullcontext()

    def _external_stream(self):
        import torch
        if self._torch_stream is not None:
            return self._torch_stream
        return torch.cuda.ExternalStream(self._stream_handle, device=self.device)

    def finish(self, raw_statuses=False):
        """-> (group_ok[groups], local statuses, left_xy[groups], right_xy[groups]); the verdict and the accumulators are those of
        the WHOLE sharded batch (identical on every rank), the statuses are this rank's proofs'."""
        self._finished = self.batch.finish_groups(raw_statuses=raw_statuses)
        return self._finished

    def finish_tensors(self):
        """finish() into device memory (Batch.finish_into), without a host wait -> dict of seven tensors on the rank's device: status
        int32 [n] (this rank's proofs), group_ok int32 [groups], left_xy / right_xy uint8 [groups, 64] (the whole sharded batch's, as
        finish() gives them), group_failed int32 [groups] (this rank's failing proofs per group), failed_index int32 [n] (their
        indices in ascending order, then -1), summary int32 [Batch.SUMMARY_WORDS].  They are written on the batch's stream and torch's
        current stream is made to wait for it on the device: work queued there afterwards sees them.  finish() may still follow."""
        import torch
        n, g, dev = self.batch.n, self.batch.groups, self.device
        out = {"status": torch.empty(n, dtype=torch.int32, device=dev), "group_ok": torch.empty(g, dtype=torch.int32, device=dev),
               "left_xy": torch.empty((g, 64), dtype=torch.uint8, device=dev), "right_xy": torch.empty((g, 64), dtype=torch.uint8, device=dev),
               "group_failed": torch.empty(g, dtype=torch.int32, device=dev), "failed_index": torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev),
               "summary": torch.empty(self.batch.SUMMARY_WORDS, dtype=torch.int32, device=dev)}
        self.batch.finish_into(**out)
        out["failed_index"] = out["failed_index"][:n]
        return out

    def identify(self, verdicts=None):
        """After finish(): which of THIS rank's proofs fail the pairing (Batch.identify) -> (local statuses, range_checks).  Local to
        the rank, no collective: a shard's own sum, sum over its proofs of (the product of all later draws of the batch) * Guard_i, is a
        random linear combination with distinct monomials, so a shard holding a bad proof fails its own pairing except with
        probability <= count / r, a shard of good proofs always passes, and the whole batch is the product of the shards' checks.  The
        rank's own accumulators are lost at the fold (it overwrites the pieces in the workspace) and survive in the record the rank
        exported: `records` is passed on whenever the launch exchanged records.
        verdicts: the groups' verdicts of the whole batch, default the last finish()'s (verify_batch_sharded_local passes the fold's,
        which only shard 0 sees).  When every one passed, the finished statuses come back with 0 range checks and nothing runs."""
        if self._finished is None:
            raise ValueError("identify() comes after finish()")
        group_ok, statuses = self._finished[0], self._finished[1]
        if isinstance(statuses, (bytes, bytearray)):
            statuses = memoryview(bytes(statuses)).cast('i').tolist()
        if all(group_ok if verdicts is None else verdicts):
            return list(statuses), 0
        st, _, checks = self.batch.identify(self.records.data_ptr() if self._exchanged else None)
        return st, checks


def _flatten(proofs, instances):
    """-> (proofs_flat, proof_len, instances_flat, col_lens); one instance shape per sharded batch (the staged interface)."""
    from .verifier import _flatten_instances
    if len(instances) != len(proofs):
        raise ValueError(f"{len(proofs)} proofs but {len(instances)} instance lists")
    plen = len(proofs[0]) if proofs else 0
    if any(len(p) != plen for p in proofs):
        raise ValueError("a sharded batch takes proofs of one length (one VerifyingKey)")
    flats, lens0 = [], None
    for inst in instances:
        f, lens = _flatten_instances(inst)
        if lens0 is None:
            lens0 = lens
        elif lens != lens0:
            raise ValueError("a sharded batch takes one instance shape (use Context.verify_batch for mixed shapes)")
        flats.append(f)
    return b"".join(bytes(p) for p in proofs), plen, b"".join(flats), lens0


def _shard(ctx, proofs, instances, lo, hi):
    """Proofs [lo, hi) of a batch in the staged form -> (proofs_flat, proof_len, instances_flat, col_lens).  An empty shard still takes
    part in the launch and the collectives: it brings the batch's proof length and instance shape, the context's for a batch of no proofs."""
    flat, plen, iflat, lens = _flatten(proofs[lo:hi], instances[lo:hi])
    if lens is None:
        lens = _flatten(proofs[:1], instances[:1])[3] if len(proofs) else [0] * ctx.proof_shape()["n_instance_columns"]
    if not plen:
        plen = len(proofs[0]) if len(proofs) else ctx.proof_shape()["proof_len"]
    return flat, plen, iflat, lens


def _hint_rows(hints, n):
    """The hints= keyword of the sharded calls: one row (bytes) or None per proof of the WHOLE batch, checked before anything runs;
    every rank then takes its own slice.  Hints are not exchanged."""
    if hints is None:
        return None
    if isinstance(hints, (bytes, bytearray, str)) or not hasattr(hints, "__len__"):
        raise TypeError("hints must be a sequence of bytes or None, one per proof")
    if len(hints) != n:
        raise ValueError(f"{n} proofs need {n} hint rows (None for a proof without hints), got {len(hints)}")
    return list(hints)


def _all_statuses(local, n, world, group, backend, device):
    """Per-proof statuses of the whole batch, in call order, on every rank (a second, 4 n-byte all-gather)."""
    if world == 1:
        return list(local)
    import torch
    import torch.distributed as dist
    per = (n + world - 1) // world
    dev = device if backend == "nccl" else "cpu"
    mine = torch.zeros(max(per, 1), dtype=torch.int32, device=dev)
    if local:
        mine[: len(local)] = torch.tensor(local, dtype=torch.int32, device=dev)
    out = torch.empty(world * max(per, 1), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(out, mine, group=group)
    out = out.cpu().tolist()
    res = []
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        res += out[r * max(per, 1): r * max(per, 1) + (hi - lo)]
    return res


def _refuse_zero_draws(draws: bytes):
    """Identification needs every multiplier non-zero (a single proof's check is SingleStrategy's only then).  Every rank holds the whole
    draw stream, so every rank refuses the same batches, before any upload: none enters a collective the others skip."""
    zero = bytes(32)
    if any(draws[i:i + 32] == zero for i in range(0, len(draws), 32)):
        raise ValueError("identification takes non-zero draws: a draw of the batch is zero")


def _seeded_draws(seed, rand, n, lo, identify, group=None, device=None):
    """The tail of a shard that starts at proof `lo` of n, from `seed` (True: common_seed; bytes: given) -> n - lo draws as bytes.
    Only the identifying forms expand the whole stream, to refuse a zero draw on every rank alike."""
    if rand is not None:
        raise ValueError("give the draws (rand) or the seed they come from, not both")
    from . import draws
    seed = _resolve_seed(seed, group, device)
    if identify:
        _refuse_zero_draws(draws.expand(seed, 0, n))
    return seed, seeded_tail(seed, lo, n)


def verify_batch_sharded(ctx, proofs, instances, rand=None, group=None, batch_factory=None, device=None, identify=False, seed=None, hints=None):
    """N x verify_proof under ONE AccumulatorStrategy followed by finalize() (lib.rs:33-425, kzg/strategy.rs:125-140) with the
    proofs sharded over the ranks of `group` (default: the world) — BASELINE.json configs 3 and 5.

    Every rank calls it with the SAME `proofs` / `instances` (the whole batch in call order; one instance shape) on its own
    Context (one per GPU).  rand: the n Fr::random draws in call order, the same on every rank — or None: rank 0 draws them from
    the OS and broadcasts.  Rank r verifies shard_bounds(n, world, r) with the draw tail of its global position, the 1312-byte
    accumulator records are all-gathered (RCCL under the nccl backend), folded, and ONE pairing closes the batch.
    -> (ok, statuses[n], left_xy, right_xy), identical on every rank and — for given draws — for every world size.
    identify: verify_batch_sharded_identify's form -> (ok, statuses[n], left_xy, right_xy, local_range_checks).
    seed (instead of rand): the draws are draws.expand(seed, 0, n) — True: rank 0 takes a seed from the OS and broadcasts its 32
    bytes (common_seed); bytes: a given seed, the same on every rank.  No n x 32-byte broadcast happens: every rank expands its own
    tail, and the result is the one of rand = those draws.
    hints: one hint row (hints.for_proofs) or None per proof of the whole batch; rank r stages the rows of its own shard
    (Batch.set_hint_rows).  The result is the one without hints."""
    rank, world, backend = _group_info(group)
    n = len(proofs)
    hints = _hint_rows(hints, n)
    if device is None and batch_factory is None:
        device = f"cuda:{ctx.device}"
    lo, hi = shard_bounds(n, world, rank)
    if seed is not None:
        tail = _seeded_draws(seed, rand, n, lo, identify, group, device)[1]
    else:
        draws = common_draws(n, rand, group, device)
        if identify:
            _refuse_zero_draws(draws)
        tail = tail_for_shard(draws, lo)
    flat, plen, iflat, lens = _shard(ctx, proofs, instances, lo, hi)
    sb = ShardedBatch(ctx, hi - lo, max(sum(lens), 1), group=group, device=device, batch_factory=batch_factory)
    try:
        sb.upload(flat, plen, iflat, lens, tail)
        if hints is not None:
            sb.set_hint_rows(hints[lo:hi])
        sb.launch()
        ok, st, left, right = sb.finish()
        checks = 0
        if identify:
            st, checks = sb.identify()
    finally:
        sb.close()
    statuses = _all_statuses(st, n, world, group, backend, sb.device)
    if identify:
        return bool(ok[0]), statuses, left[0], right[0], checks
    return bool(ok[0]), statuses, left[0], right[0]


def verify_batch_sharded_identify(ctx, proofs, instances, rand=None, group=None, batch_factory=None, device=None, seed=None):
    """verify_batch_sharded plus the proofs that made it fail.  -> (ok, statuses[n], left_xy, right_xy, local_range_checks): ok / left_xy /
    right_xy are verify_batch_sharded's, statuses[i] is what Context.verify_each returns for proof i — identical on every rank and for
    every world size — and local_range_checks is the number of range checks THIS rank's search ran (0 on a rank whose shard is clean, and
    everywhere when the batch passes).  Every rank searches its own shard (ShardedBatch.identify) before the status all-gather that
    verify_batch_sharded ends with; no other collective is added.  A zero among the common draws raises ValueError on every rank before
    any upload."""
    return verify_batch_sharded(ctx, proofs, instances, rand, group, batch_factory, device, identify=True, seed=seed)


def verify_batch_sharded_local(ctx, proofs, instances, rand=None, world: int = 1, batch_factory=None, device=None, identify=False, seed=None, hints=None):
    """The `world`-rank computation of verify_batch_sharded run shard after shard on ONE device, no process group: every shard is
    uploaded with the draw tail of its global position and launched without a pairing, the records are laid out as the all-gather
    would, shard 0 folds them and runs the one pairing.  -> (ok, statuses[n], left_xy, right_xy).
    identify: verify_batch_sharded_local_identify's form -> (ok, statuses[n], left_xy, right_xy, range_checks[world]).
    seed (instead of rand): verify_batch_sharded's — every shard's tail is expanded from the seed on its own.
    hints: verify_batch_sharded's — shard r stages the rows [lo, hi) of its own proofs."""
    import torch
    n = len(proofs)
    hints = _hint_rows(hints, n)
    if rand is not None and len(rand) != n:
        raise ValueError(f"rand must hold one scalar per proof ({n}), got {len(rand)}")
    if seed is not None:
        seed = _seeded_draws(seed, rand, n, n, identify)[0]
        tail_of = lambda lo: seeded_tail(seed, lo, n)
    else:
        draws = _scalar_bytes(rand) if rand is not None else draw_scalars(n)
        if identify:
            _refuse_zero_draws(draws)
        tail_of = lambda lo: tail_for_shard(draws, lo)
    if device is None and batch_factory is None:
        device = f"cuda:{ctx.device}"
    shards, statuses = [], []
    try:
        for r in range(world):
            lo, hi = shard_bounds(n, world, r)
            flat, plen, iflat, lens = _shard(ctx, proofs, instances, lo, hi)
            sb = ShardedBatch(ctx, hi - lo, max(sum(lens), 1), device=device, batch_factory=batch_factory, world_size=world)
            shards.append(sb)
            sb.upload(flat, plen, iflat, lens, tail_of(lo))
            if hints is not None:
                sb.set_hint_rows(hints[lo:hi])
            sb.launch_shard()
            _, st, _, _ = sb.finish()
            statuses += st
        gathered = torch.cat([sb.records for sb in shards])
        if gathered.device.type == "cuda":
            torch.cuda.synchronize(gathered.device)
        shards[0].fold(gathered, world)
        ok, _, left, right = shards[0].finish()
        checks = []
        if identify:   # every shard searches its own proofs, told the verdict of the whole batch
            statuses = []
            for sb in shards:
                st, c = sb.identify(verdicts=ok)
                statuses += st
                checks.append(c)
    finally:
        for sb in shards:
            sb.close()
    if identify:
        return bool(ok[0]), statuses, left[0], right[0], checks
    return bool(ok[0]), statuses, left[0], right[0]


def verify_batch_sharded_local_identify(ctx, proofs, instances, rand=None, world: int = 1, batch_factory=None, device=None, seed=None):
    """verify_batch_sharded_identify's computation in verify_batch_sharded_local's sequential one-GPU form.
    -> (ok, statuses[n], left_xy, right_xy, range_checks[world]): the range checks every shard's search ran, shard by shard."""
    return verify_batch_sharded_local(ctx, proofs, instances, rand, world, batch_factory, device, identify=True, seed=seed)


# ---------------------------------------------------------------------------------------------------------------- streaming form
def _refuse_zero_merge_draws(draws: bytes):
    """A zero draw would drop its rank's accumulator from the merged check.  Every rank holds the whole draw stream, so every rank
    refuses the same draws at the same point: none enters a collective the others skip."""
    zero = bytes(32)
    if any(draws[i:i + 32] == zero for i in range(0, len(draws), 32)):
        raise ValueError("a merge takes non-zero draws: a draw is zero")


def _gather_bytes(mine: bytes, world, group, backend, device):
    """all_gather of one fixed-length byte string per rank -> the list of them in rank order"""
    if world == 1:
        return [mine]
    import torch
    import torch.distributed as dist
    dev = device if (backend == "nccl" and device is not None) else "cpu"
    local = torch.frombuffer(bytearray(mine), dtype=torch.uint8).to(dev)
    out = torch.empty(world * len(mine), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, local, group=group)
    flat = bytes(out.cpu().numpy().tobytes())
    return [flat[r * len(mine):(r + 1) * len(mine)] for r in range(world)]


def _merge_states(ctx, states, draws: bytes, accumulator_factory):
    """A fresh accumulator with a journal of len(states) + 1 entries, the states merged into it in order: entry 1 + k is state k."""
    merged = accumulator_factory(ctx, len(states) + 1)
    try:
        merged.merge_states(states, [draws[32 * k:32 * k + 32] for k in range(len(states))])
    except Exception:
        merged.close()
        raise
    return merged


def _default_accumulator(ctx, journal):
    from .verifier import Accumulator
    return Accumulator(ctx, journal=journal)


class ShardedAccumulator:
    """A resident accumulator per rank of a torch.distributed group (one process per GPU), closed by ONE pairing.

    Every rank feeds `acc` (an Accumulator over the rank's own Context) with its own proofs: acc.process(...) — no collective runs
    per leg.  finalize() all-gathers the ranks' exported states (152 bytes each), takes one draw per rank — rank 0 draws them from
    the OS and broadcasts (common_draws) — and merges all states in rank order into a fresh accumulator with a journal of
    world + 1 entries: (L, R) = sum_k c_k (L_k, R_k), the counters added.  Every rank computes the same merge and gets the same
    (ok, left_xy, right_xy) bit for bit.  check_ranks() then returns the merged journal's pairing bit per rank: a rank whose own
    accumulator is poisoned shows 0 (c_k != 0: the entry's bit is the rank's own bit).  The ranks' accumulators are not changed and go
    on accumulating afterwards.

    At construction the ranks compare a hash of their params bytes once (a state carries no SRS, so the merge cannot check it): a
    mismatch raises ValueError on every rank.
    accumulator_factory(ctx, journal) builds the accumulators; the default is verifier.Accumulator (the non-GPU test suite injects a
    stand-in to exercise the orchestration over gloo)."""

    def __init__(self, ctx, group=None, device=None, accumulator_factory=None):
        self.rank, self.world, self.backend = _group_info(group)
        self.group, self.ctx = group, ctx
        if accumulator_factory is None:
            accumulator_factory = _default_accumulator
            if device is None:
                device = f"cuda:{ctx.device}"
        self.device = device
        self._factory = accumulator_factory
        digest = hashlib.sha256(bytes(ctx.params.data)).digest()
        if len(set(_gather_bytes(digest, self.world, group, self.backend, device))) != 1:
            raise ValueError("the ranks of a sharded accumulator hold different params")
        self.acc = accumulator_factory(ctx, 0)
        self.merged = None
        self.last_draws = None

    def close(self):
        for a in (self.acc, self.merged):
            if a is not None:
                a.close()
        self.acc = self.merged = None

    def process(self, *args, **kwargs):
        """Accumulator.process on this rank's accumulator"""
        return self.acc.process(*args, **kwargs)

    def finalize(self, draws=None):
        """-> (ok, left_xy, right_xy) of the merge of every rank's accumulator, identical on every rank.  draws: one non-zero scalar
        per rank, the same on every rank (tests), or None: rank 0 draws them and broadcasts.  A zero draw raises ValueError on every rank."""
        states = _gather_bytes(self.acc.export_state(), self.world, self.group, self.backend, self.device)
        c = common_draws(self.world, draws, self.group, self.device)
        _refuse_zero_merge_draws(c)
        if self.merged is not None:
            self.merged.close()
            self.merged = None
        self.merged = _merge_states(self.ctx, states, c, self._factory)
        self.last_draws = c
        return self.merged.finalize()

    def check_ranks(self):
        """After finalize(): the pairing bit of every rank's own accumulator, [1, 0, ..] in rank order (the merged journal's entries
        1 .. world; one launch, no collective: every rank holds the merged journal)."""
        if self.merged is None:
            raise ValueError("check_ranks() comes after finalize()")
        return [int(ok) for _, _, ok in self.merged.check_legs()[1:]]


def merge_accumulators_local(ctx, accumulators, draws=None, accumulator_factory=None):
    """ShardedAccumulator.finalize()'s computation over accumulators of ONE GPU (no process group): their exported states merged in
    order into a fresh accumulator with a journal, one draw each (None: OS draws).  For callers with several feeder threads, each with
    an accumulator of its own, and for tests.  -> (ok, left_xy, right_xy, bits): bits[k] = the pairing bit of accumulators[k] alone."""
    accumulators = list(accumulators)
    c = common_draws(len(accumulators), draws) if draws is not None else draw_scalars(len(accumulators))
    _refuse_zero_merge_draws(c)
    merged = _merge_states(ctx, [a.export_state() for a in accumulators], c, accumulator_factory or _default_accumulator)
    try:
        ok, left, right = merged.finalize()
        return ok, left, right, [int(b) for _, _, b in merged.check_legs()[1:]]
    finally:
        merged.close()
