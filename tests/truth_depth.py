"""
TEST INFRASTRUCTURE: --truth-depth restated in plain Python (README, "True coverage").

depth(contig, p) = the PAF records with tname = contig and tstart <= p < tend.  `bedgraph_from_paf` builds it the slow, obvious way: a
numpy difference array per contig (+1 at tstart, -1 at tend), its running sum, and the maximal runs of equal depth as lines
`contig TAB start TAB end TAB depth LF`, zero runs included, every contig from 0 to its length in reference order.
`bedgraph_from_events` does the same from the device's events (include/brx.h: BRX_DEPTH_EVENT), `events_from_paf` makes the events a
PAF text stands for, `check_bedgraph` checks a file without either.
"""
import numpy as np

POS_BITS = 39


def event(contig, pos, is_start):
    return (int(contig) << 40) | (int(pos) << 1) | int(bool(is_start))


def paf_intervals(paf_text, names):
    """[(contig index, tstart, tend)] of every PAF line, in line order."""
    index = {n: i for i, n in enumerate(names)}
    out = []
    for line in paf_text.splitlines():
        f = line.split('\t')
        out.append((index[f[5]], int(f[7]), int(f[8])))
    return out


def events_from_paf(paf_text, names):
    """The uint64 events of brx_emit_depth for these PAF lines: per line the start event, then the end event."""
    ev = []
    for c, s, e in paf_intervals(paf_text, names):
        ev += [event(c, s, 1), event(c, e, 0)]
    return np.array(ev, dtype=np.uint64)


def intervals_of_events(events):
    """(contig, position, +1 / -1) arrays of uint64 events."""
    ev = np.asarray(events, dtype=np.uint64)
    contig = (ev >> np.uint64(40)).astype(np.int64)
    pos = ((ev >> np.uint64(1)) & np.uint64((1 << POS_BITS) - 1)).astype(np.int64)
    delta = np.where(ev & np.uint64(1), 1, -1).astype(np.int64)
    return contig, pos, delta


def _bedgraph(contig, pos, delta, names, lengths):
    lines = []
    for c, (name, length) in enumerate(zip(names, lengths)):
        length = int(length)
        diff = np.zeros(length + 1, dtype=np.int64)
        mine = contig == c
        np.add.at(diff, pos[mine], delta[mine])
        depth = np.cumsum(diff[:length])
        assert diff.sum() == 0 and (depth >= 0).all()
        if length == 0:
            continue
        cuts = np.flatnonzero(depth[1:] != depth[:-1]) + 1
        starts = np.concatenate([[0], cuts])
        ends = np.concatenate([cuts, [length]])
        lines += [f'{name}\t{s}\t{e}\t{depth[s]}\n' for s, e in zip(starts.tolist(), ends.tolist())]
    return ''.join(lines)


def bedgraph_from_events(events, names, lengths):
    contig, pos, delta = intervals_of_events(events)
    return _bedgraph(contig, pos, delta, names, lengths)


def bedgraph_from_paf(paf_text, names, lengths):
    return bedgraph_from_events(events_from_paf(paf_text, names), names, lengths)


def parse_bedgraph(text):
    rows = []
    for line in text.split('\n')[:-1]:
        name, s, e, d = line.split('\t')
        assert str(int(s)) == s and str(int(e)) == e and str(int(d)) == d, line        # plain decimals
        rows.append((name, int(s), int(e), int(d)))
    assert text == '' or text.endswith('\n')
    return rows


def check_bedgraph(text, names, lengths, paf_text=None):
    """Contigs in reference order, each tiled from 0 to its length by lines whose neighbours differ in depth; with `paf_text`, the covered
    bases equal the bases of its records.  Returns the covered bases (the sum of depth * (end - start))."""
    rows = parse_bedgraph(text)
    at = 0
    for name, length in zip(names, lengths):
        if int(length) == 0:
            continue
        pos, last = 0, None
        while at < len(rows) and rows[at][0] == name and pos < int(length):
            _, s, e, d = rows[at]
            assert s == pos and e > s and d >= 0 and d != last, rows[at]
            pos, last = e, d
            at += 1
        assert pos == int(length), (name, pos, length)
    assert at == len(rows)
    covered = sum(d * (e - s) for _, s, e, d in rows)
    if paf_text is not None:
        assert covered == sum(e - s for _, s, e in paf_intervals(paf_text, names))
    return covered


def per_base(text, names, lengths):
    """{contig: the depth of every base} of a bedGraph text."""
    out = {n: np.zeros(int(l), dtype=np.int64) for n, l in zip(names, lengths)}
    for name, s, e, d in parse_bedgraph(text):
        out[name][s:e] = d
    return out
