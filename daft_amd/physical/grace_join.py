"""Out-of-core hash join: grace partitioning (ref: the partitioned execution
the reference uses to join inputs many times larger than memory).

JoinOp hands over here when its build side exceeds the operator budget and
has been spilled to host.  Both inputs are split by a hash of the join key
into `nb` host-resident buckets, so that rows which can match share a
bucket; bucket p of the build side is then loaded into HBM and joined with
bucket p of the probe side by the in-memory join, one bucket at a time.

Limits:
  * at most 256 partitions (one pass of the native partitioner,
    csrc/partition.hip);
  * no recursive repartitioning: a build bucket that is still over budget
    (one very frequent key, or nb capped at 256) is joined in memory as it
    is and counted in `grace_stats["oversize_buckets"]`;
  * the output is bucket-major: rows come out in an order that differs from
    the in-memory join's.  Only inputs that could not run at all before take
    this path.
"""
from __future__ import annotations

from typing import Iterator, List

from ..kernels import rowops
from ..recordbatch import RecordBatch
from ..schema import supertype

MAX_PARTITIONS = 256


def num_partitions(total_build_bytes: int, budget: int) -> int:
    """Buckets sized to a quarter of the budget, as in the external sort:
    that leaves room for the hash table, a probe slice and the output."""
    nb = -(-int(total_build_bytes) // max(int(budget) // 4, 1))
    return max(2, min(nb, MAX_PARTITIONS))


def _key_dtypes(op) -> list:
    """Per key pair, the type rowops.join compares in."""
    lschema, rschema = op.children[0].schema, op.children[1].schema
    return [supertype(le.to_field(lschema).dtype, re.to_field(rschema).dtype)
            for le, re in zip(op.left_on, op.right_on)]


def _partition(rb: RecordBatch, exprs, dtypes, nb: int):
    """(rows of `rb` grouped by bucket, rows per bucket)."""
    keys = []
    for e, st in zip(exprs, dtypes):
        k = e.evaluate(rb)
        if k.is_dict():
            k = k.dict_decode()
        keys.append(k.cast(st) if k.dtype != st else k)
    # Rows that rowops.join would match must land in the same bucket on
    # both sides, so both sides hash the VALUE in the join's comparison
    # type: hash_columns alone hashes 4- and 8-byte integers differently
    # and dictionary columns by their per-vocabulary codes.
    #
    # remix=True is required, not cosmetic.  The bucket's hash table
    # (join_build) indexes with the low bits of this same row hash; for a
    # single key column a different seed only XORs a constant into it, so
    # it does not decorrelate the two.  With plain h % nb and nb a power of
    # two, every row of a bucket would share its low hash bits and the
    # bucket's table would use 1/nb of its slots.  splitmix64 before the
    # modulo breaks that.
    h = rowops.hash_values(keys)
    perm, counts = rowops.hash_partition(h, nb, remix=True)
    return rb.take(perm, has_neg=False), counts.tolist()


def _scatter_to_host(rb: RecordBatch, exprs, dtypes, nb: int,
                     buckets: List[List[RecordBatch]]) -> None:
    if len(rb) == 0:
        return
    reordered, counts = _partition(rb, exprs, dtypes, nb)
    off = 0
    for p, c in enumerate(counts):
        if c:
            buckets[p].append(reordered.slice(off, off + c).cpu())
        off += c


def _load(parts: List[RecordBatch], schema, device) -> RecordBatch:
    if not parts:
        return RecordBatch.empty(schema, device=device)
    return RecordBatch.concat([p.to(device) for p in parts])


def run_grace_join(op, ectx, spilled: List[RecordBatch],
                   budget: int) -> Iterator[RecordBatch]:
    """Join `op` (a JoinOp, any `how` but cross) whose build side lies in
    the host runs `spilled`.  Output is bucket-major (see module docstring)."""
    from .ops import stream_host_batch
    how = op.how
    device = ectx.device
    build_bytes = sum(r.size_bytes() for r in spilled)
    nb = num_partitions(build_bytes, budget)
    dtypes = _key_dtypes(op)
    ectx.op_names[id(op)] = f"{op.op_name} grace({nb})"
    morsel = getattr(ectx.ctx.execution_config, "stream_morsel_rows",
                     1 << 26)

    build_buckets: List[List[RecordBatch]] = [[] for _ in range(nb)]
    while spilled:
        run = spilled.pop(0)
        for mo in stream_host_batch(run, device, morsel):
            _scatter_to_host(mo, op.right_on, dtypes, nb, build_buckets)
        del run
    probe_buckets: List[List[RecordBatch]] = [[] for _ in range(nb)]
    for left in op.children[0].execute_tracked(ectx):
        _scatter_to_host(left, op.left_on, dtypes, nb, probe_buckets)

    sizes = [sum(b.size_bytes() for b in parts) for parts in build_buckets]
    op.grace_stats = {
        "partitions": nb,
        "build_bytes": int(build_bytes),
        "max_build_bucket_bytes": int(max(sizes)),
        "oversize_buckets": sum(1 for s in sizes if s > budget),
    }

    lschema, rschema = op.children[0].schema, op.children[1].schema
    for p in range(nb):
        bparts, pparts = build_buckets[p], probe_buckets[p]
        build_buckets[p] = probe_buckets[p] = None   # release host copies
        if not bparts and not pparts:
            continue
        right = _load(bparts, rschema, device)
        del bparts
        rkeys = [e.evaluate(right) for e in op.right_on]
        if how in ("inner", "left", "semi", "anti"):
            # the probe bucket streams through slice by slice
            while pparts:
                left = pparts.pop(0).to(device)
                lkeys = [e.evaluate(left) for e in op.left_on]
                lidx, ridx = rowops.join(lkeys, rkeys, how)
                if how in ("semi", "anti"):
                    yield left.take(lidx)
                else:
                    yield op._emit(left, right, lidx, ridx)
        else:
            # right/outer track unmatched build rows over the whole bucket
            left = _load(pparts, lschema, device)
            del pparts
            lkeys = [e.evaluate(left) for e in op.left_on]
            lidx, ridx = rowops.join(lkeys, rkeys, how)
            yield op._emit(left, right, lidx, ridx)
        del right, rkeys
