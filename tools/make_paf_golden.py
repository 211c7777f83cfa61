#!/usr/bin/env python3
"""
Generate tests/golden/paf_lines.json.gz by RUNNING THE UNMODIFIED REFERENCE (/root/reference, Badread 0.4.2): its
badread.alignment.Alignment over PAF lines that brx_paf_scan must flag as irregular (include/brx.h: BRX_PAF_IRREGULAR) and hand to the
host.  For every line the fixture records its name, the line itself and either every attribute of the reference's object, `repr` and
`cigar_parts` (the reference keeps them as text, '10M') among them, or how the reference ended: the message of its sys.exit, or the
type of the exception it raised.  `regular` is the plain line the others are variations of.

Deterministic: a second run changes no byte.  Run:  python tools/make_paf_golden.py   (needs /root/reference; instant)
"""
import gzip
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
for p in (os.path.join(REPO, 'oracle', 'shim'), REFERENCE):
    if p not in sys.path:
        sys.path.insert(0, p)

import badread.alignment as ref_alignment                  # noqa: E402  (the reference)
import badread.version as ref_version                      # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'paf_lines.json.gz')
FIELDS = ['odd', '400', '5', '305', '+', 'ctg', '5000', '1000', '1310', '290', '312', '60', 'tp:A:P', 'AS:i:540', 'cg:Z:100M2I10D198M']
ATTRIBUTES = ('read_name', 'read_start', 'read_end', 'strand', 'ref_name', 'ref_start', 'ref_end', 'matching_bases', 'num_bases',
              'percent_identity', 'cigar', 'alignment_score', 'max_indel', 'cigar_parts')


def line(**changes):
    """The regular line with some fields replaced (by index: f4='+-') or dropped (None)."""
    fields = list(FIELDS)
    for key, value in changes.items():
        fields[int(key[1:])] = value
    return '\t'.join(f for f in fields if f is not None)


def with_cigar(cigar):
    return line(f14='cg:Z:' + cigar)


ODD = [
    ('leading_blank', ' ' + line()),
    ('trailing_tab', line() + '\t'),
    ('blank_in_name', line(f0='odd read')),
    ('empty_line', ''),
    ('ten_fields', '\t'.join(FIELDS[:10])),
    ('no_cg', line(f14=None)),
    ('no_as', line(f13=None)),
    ('strand_plus_minus', line(f4='+-')),
    ('strand_plus_five', line(f4='+5')),
    ('integer_19_digits', line(f8='1000000000000000000')),
    ('num_bases_zero', line(f10='0')),
    ('cg_empty', with_cigar('')),
    ('cigar_eq_x', with_cigar('10=5X285M')),
    ('cigar_trailing_digits', with_cigar('300M5M3')),
    ('cigar_two_letters', with_cigar('300M5MM')),
    ('cigar_underscore', with_cigar('300M5_')),
    ('cigar_10_digit_length', with_cigar('300M1234567890D')),
    ('cigar_minus_strand', line(f4='-', f14='cg:Z:10=5X200M3D85M')),
]


def record(name, text):
    try:
        a = ref_alignment.Alignment(text + '\n')
    except SystemExit as e:
        return dict(name=name, line=text, exit=str(e.code))
    except Exception as e:                                 # noqa: BLE001  (what the reference raises is what is recorded)
        return dict(name=name, line=text, exception=type(e).__name__)
    got = {k: getattr(a, k) for k in ATTRIBUTES}
    got['percent_identity'] = repr(got['percent_identity'])
    return dict(name=name, line=text, attributes=got, repr=repr(a))


def main():
    doc = dict(reference_version=ref_version.__version__, regular=record('regular', line()), odd=[record(n, t) for n, t in ODD])
    assert 'attributes' in doc['regular']
    with gzip.GzipFile(OUT, 'wb', mtime=0) as f:
        f.write(json.dumps(doc, indent=1, sort_keys=True).encode())
    print(OUT, len(doc['odd']), 'lines')


if __name__ == '__main__':
    main()
