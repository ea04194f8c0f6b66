"""Analyse a per-segment debug timeline (AIRS_DBG bit 65536 dump of an
ablation build): slots 0 start, 1 aggregate published, 2 look-back done,
3 look-back start, 4 segment done (wave 0), 5 look-back rounds | retries
<< 32, 6 tail re-polls, 7 hw id.  Times in us (realtime clock, 100 MHz).
usage: ts_analyze.py FILE SEGS_PER_FRAME
       ts_analyze.py FILE SEGS_PER_FRAME --front [RING]

--front: the light timeline with the entry stamp (AIRS_DBG
65536 | 131072 | 262144): slot 1 = the shader clock at slot 0, slot 2 = at
slot 4, slot 3 = the shader clock at the kernel's entry, slot 5 = wave 0's
samples landed.  Prints entry -> slot 0 (shader cycles, and ns at the
launch's clock) and slot 0 -> samples landed (us), median and p90, for the
first generation of workgroups (block index below 1536: six per CU on 256 CUs)
and for the rest; FILE holds RING launches (AIRS_DBGTS_RING, default 1), the
figures are over every launch but the first."""
import sys

import numpy as np


def front(path, spf, ring):
    raw = np.fromfile(path, dtype=np.uint64)
    a_all = raw.reshape(ring, -1, 8).astype(np.int64)
    # (the array is sized for the caller's 4096-sample segments; the Rice
    # kernel stamps one entry per 16 Ki-sample segment, the first ones)
    a_all = a_all[:, :int(np.nonzero((a_all[:, :, 0] > 0).any(axis=0))[0].max()) + 1]
    nseg = a_all.shape[1]
    nfr = nseg // spf
    g = np.arange(nseg)
    blk = (g % spf) * nfr + g // spf  # frame-interleaved order: block = sif nfr + lf
    rows = {"first generation (blocks < 1536)": blk < 1536, "later generations": blk >= 1536}
    acc = {k: dict(cyc=[], ns=[], land=[]) for k in rows}
    mhz_all = []
    for r in range(1 if ring > 1 else 0, ring):
        a = a_all[r]
        ok = (a[:, 0] > 0) & (a[:, 4] > a[:, 0]) & (a[:, 3] > 0) & (a[:, 1] >= a[:, 3])
        if not ok.any():
            continue
        dt = (a[:, 4] - a[:, 0]) / 100.0  # us
        mhz = float(np.median((a[ok, 2] - a[ok, 1]) / dt[ok]))
        mhz_all.append(mhz)
        cyc = (a[:, 1] - a[:, 3]).astype(float)
        land = np.where(a[:, 5] > 0, (a[:, 5] - a[:, 0]) / 100.0, np.nan)
        for k, sel in rows.items():
            m = ok & sel
            acc[k]["cyc"].append(cyc[m])
            acc[k]["ns"].append(cyc[m] / mhz * 1e3)
            acc[k]["land"].append(land[m])
    print(f"launches {len(mhz_all)}  segments {nseg}  frames {nfr}  shader clock median {np.median(mhz_all):.0f} MHz")
    print(f"{'':34} {'entry->slot 0, cycles':>24} {'entry->slot 0, ns':>20} {'slot 0->landed, us':>20}")
    for k, v in acc.items():
        c, n, ld = (np.concatenate(v[x]) if v[x] else np.array([np.nan]) for x in ("cyc", "ns", "land"))
        f = lambda x, w: f"{np.nanmedian(x):{w}} / {np.nanpercentile(x, 90):{w}}"  # noqa: E731
        print(f"{k:<34} {f(c, '9.0f'):>24} {f(n, '7.0f'):>20} {f(ld, '6.2f'):>20}   (median / p90, n = {len(c)})")


if "--front" in sys.argv:
    i = sys.argv.index("--front")
    front(sys.argv[1], int(sys.argv[2]), int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 1)
    sys.exit(0)

a = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, 8).astype(np.int64)
spf = int(sys.argv[2])
nf = len(a) // spf
ok = a[:, 0] > 0
base = a[ok, 0].min()
t = np.where(a[:, :5] > 0, (a[:, :5] - base) / 100.0, np.nan)
st, ag, lbd, lbs, end = (t[:, i] for i in range(5))
R = lambda x: f"{np.nanmedian(x):6.2f}/{np.nanpercentile(x, 90):6.2f}"  # noqa: E731
print(f"segments {len(a)} frames {nf} kernel span {np.nanmax(end):.1f} us  (median/p90 us)")
print(f" start->agg {R(ag - st)}  start->LBstart {R(lbs - st)}  LB wait {R(lbd - lbs)}  "
      f"LBdone->end {R(end - lbd)}  residency {R(end - st)}")
T = lambda x: x.reshape(nf, spf)  # noqa: E731
ag2, lbs2, lbd2, st2 = T(ag), T(lbs), T(lbd), T(st)
print(f" pred agg later than succ LB start: {np.nanmean(ag2[:, :-1] > lbs2[:, 1:]) * 100:.1f}%   "
      f"pred LB done later than succ LB start: {np.nanmean(lbd2[:, :-1] > lbs2[:, 1:]) * 100:.1f}%")
# occupancy over time
grid = np.arange(0, np.nanmax(end), 1.0)
act = [int(((st <= g) & (end > g)).sum()) for g in grid]
wait = [int(((lbs <= g) & (lbd > g)).sum()) for g in grid]
step = max(1, len(grid) // 25)
print(" resident per us:", act[::step])
print(" in LB wait per us:", wait[::step])
nf_ = a[:, 5] & 0xFFFFFFFF
rt = a[:, 5] >> 32
m = lbs >= 0
print(f" LB rounds: mean {nf_[m].mean():.2f} max {nf_[m].max()}  retries: mean {rt[m].mean():.2f}  "
      f"tail re-polls: mean {a[m, 6].mean():.2f} (>0 in {np.mean(a[m, 6] > 0) * 100:.1f}%)")
for r in (1, 2, 3):
    sel = m & (nf_ == r)
    if sel.any():
        print(f"  rounds={r}: {sel.sum()} segs, LB wait {R(lbd[sel] - lbs[sel])}")
sel = m & (nf_ == 1) & (a[:, 6] == 0)
if sel.any():
    print(f"  1 round, no tail re-poll: {sel.sum()} segs, LB wait {R(lbd[sel] - lbs[sel])}")
