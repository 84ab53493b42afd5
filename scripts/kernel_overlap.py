"""Kernels of a rocprofv3 --kernel-trace rocpd database that overlap in time with kernels whose name contains a substring (default
"sf16": the split-f16 training convolutions of train_ops.conv_arithmetic("split_f16")).  Usage: kernel_overlap.py <db> [substring]
Prints each overlapping kernel name once with its count; the f16 MFMA kernels must not share the GPU with ATen kernels
(packed-fp32 hazard, profiles/r06_packed_fp32_hazard.md)."""
import bisect, collections, re, sqlite3, sys

db = sqlite3.connect(sys.argv[1])
sub = sys.argv[2] if len(sys.argv) > 2 else "sf16"
cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
scol = next((c for c in ("stream_id", "queue_id", "stream", "queue") if c in cols), None)     # kernels of one stream are serialised
rows = [(s, e, re.sub(r"\(anonymous namespace\)::|^void ", "", n).split("(")[0][:100], q)
        for n, s, e, q in db.execute(f"select name, start, end, {scol or 0} from kernels order by start")]
starts = [r[0] for r in rows]
hits, worst, n_sub = collections.Counter(), collections.defaultdict(float), 0
for s, e, name, q in rows:
    if sub not in name:
        continue
    n_sub += 1
    i = bisect.bisect_left(starts, e)                 # kernels that start before this one ends ...
    for s2, e2, name2, q2 in rows[max(0, i - 512):i]:
        if e2 > s and (s2, e2, name2, q2) != (s, e, name, q):  # ... and end after it starts
            key = (name2, "same stream" if (scol and q2 == q) else "other stream")
            hits[key] += 1
            worst[key] = max(worst[key], (min(e, e2) - max(s, s2)) / 1e3)
print(f"{n_sub} kernels matching {sub!r} (stream column: {scol}); kernels overlapping them in time: {len(hits)}")
for (name, where), c in hits.most_common():
    print(f"  n={c:6d}  {where:12s}  longest overlap {worst[(name, where)]:8.2f} us  {name}")
