"""Idle time of the main stream per proof period of a queue, from a rocprofv3 --kernel-trace run (rocpd sqlite .db).

The main stream is the queue `qap_kernel` runs on; a period runs from one proof's qap_kernel to the next one's.  Per
period: its length, the sum of the main stream's kernels, the idle remainder, the gap in front of qap_kernel (the end
of the last proof's H accumulation -> the next proof's first kernel), the gap behind it (-> the next kernel on that
stream, whatever it is) and the largest other gap; then the medians and the median launch-to-launch spacing of the
stream, against which a gap counts as gone.
usage: python tools/main_stream_idle.py results.db [skip_first_periods] [out.md]"""
import sqlite3
import statistics
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    cur = db.cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table','view')")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    cols = [r[1] for r in cur.execute("pragma table_info(%s)" % kd)]
    qcol = "queue_id" if "queue_id" in cols else ("stream_id" if "stream_id" in cols else "0")
    rows = list(cur.execute("select d.start, d.end, d.%s, s.kernel_name from %s d join %s s on d.kernel_id=s.id "
                            "order by d.start" % (qcol, kd, ks)))
    main_q = [q for _, _, q, name in rows if "qap_kernel" in name][-1]
    ms = [(st, en, name) for st, en, q, name in rows if q == main_q]
    qaps = [i for i, r in enumerate(ms) if "qap_kernel" in r[2]][skip:]
    lines = ["| period | length us | main busy us | idle us | gap before qap us | gap behind qap us | next largest gap us "
             "(in front of) |", "|---|---|---|---|---|---|---|"]
    stats, all_gaps = [], []
    for n, (i, j) in enumerate(zip(qaps[:-1], qaps[1:])):
        if i == 0:
            continue
        length = (ms[j][0] - ms[i][0]) / 1e3
        busy = sum(en - st for st, en, _ in ms[i:j]) / 1e3
        gaps = [(max(0, ms[k + 1][0] - ms[k][1]) / 1e3, ms[k + 1][2]) for k in range(i, j)]
        before = max(0, ms[i][0] - ms[i - 1][1]) / 1e3       # belongs to the period that ends here; shown with this one
        behind = gaps[0][0]
        rest = sorted(gaps[1:-1], reverse=True)[:1] or [(0.0, "-")]
        all_gaps += [g for g, _ in gaps[1:-1]]
        stats.append((length, busy, length - busy, before, behind))
        lines.append("| %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f (`%s`) |" %
                     (n + skip, length, busy, length - busy, before, behind, rest[0][0], rest[0][1].split("(")[0][-40:]))
    if stats:
        med = [statistics.median(c) for c in zip(*stats)]
        lines.append("| median of %d | %.1f | %.1f | %.1f | %.1f | %.1f | |" % ((len(stats),) + tuple(med)))
        lines.append("")
        lines.append("median launch-to-launch spacing of the other kernels on the main stream: %.1f us"
                     % statistics.median(all_gaps))
    text = "\n".join(lines)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
