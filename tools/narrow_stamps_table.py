import re, sys, statistics as st
# per-evaluation cycles of the six intervals from a stamped k_step3b run (6 evaluations per launch), median over launches
# (the wide-product rows need a build that stamps them: older builds print no such fields and get no such rows)
rows = {0: [], 5: []}
for line in open(sys.argv[1]):
    m = re.match(r"k_step3b wave (\d) total (\d+) .*F1 (\d+)\+(\d+) F2 (\d+)\+(\d+) F3 (\d+)\+(\d+) B3 (\d+)\+(\d+) B2 (\d+)\+(\d+) B1 (\d+)\+(\d+) \| narrow.*F3 (\d+) B1 (\d+)(?: \| wide.*F2 (\d+) (\d+) B2 (\d+) (\d+))?", line)
    if m:
        v = [int(x) for x in m.groups() if x is not None]
        rows[v[0]].append(v[1:])
names = ["launch total", "0 F1 (W1 x)", "  wait", "1 F2 (W2 h1)", "  wait", "2 F3 (W3 h2, narrow, waves 0-3)", "  wait", "3 B3 (W3^T g3)", "  wait",
         "4 B2 (W2^T g2)", "  wait", "5 B1 (W1^T g1, narrow, waves 4-7)", "  wait", "narrow F3: barrier exit -> last MFMA issued", "narrow B1: barrier exit -> last MFMA issued",
         "wide F2: barrier exit -> last MFMA of half a issued", "wide F2: from there -> last MFMA of half b issued",
         "wide B2: barrier exit -> last MFMA of half a issued", "wide B2: from there -> last MFMA of half b issued"]
print(f"{'cycles per evaluation (median of %d launches)' % len(rows[0]):58s} {'wave 0':>8s} {'wave 5':>8s}")
for i, n in enumerate(names[:min(len(r) for w in (0, 5) for r in rows[w])]):
    a = [st.median(r[i] for r in rows[w]) / (1 if i == 0 else 6) for w in (0, 5)]
    print(f"{n:58s} {a[0]:8.0f} {a[1]:8.0f}")
for w in (0, 5):
    print(f"wave {w}: the six intervals and their waits sum to {sum(st.median(r[i] for r in rows[w]) for i in range(1, 13)) / 6:.0f} cycles per evaluation")
