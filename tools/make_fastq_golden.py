#!/usr/bin/env python3
"""
Generate tests/golden/fastq_texts.json.gz by RUNNING THE UNMODIFIED REFERENCE (/root/reference, Badread 0.4.2): its badread.misc.load_fastq
at dot_interval=3 over small FASTQ texts -- those of the regular layout, which brx_fastq_scan (include/brx.h) parses on the device, and
those it must hand to the host (a layout bit).  For every text the fixture records its name, its bytes (base64), the text the reference
wrote on `output`, and either the items of the returned dict in order or the type name of the exception the reference raised.

Deterministic: a second run changes no byte.  Run:  python tools/make_fastq_golden.py   (needs /root/reference; instant)
"""
import base64
import gzip
import io
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
for p in (os.path.join(REPO, 'oracle', 'shim'), REFERENCE):
    if p not in sys.path:
        sys.path.insert(0, p)

import badread.misc as ref_misc                            # noqa: E402  (the reference)
import badread.version as ref_version                      # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'fastq_texts.json.gz')
E = 'ré'.encode('utf-8')                              # two bytes of 0x80 or more

REGULAR = [
    ('single', b'@only\nACGT\n+\n!!!!\n'),
    ('crlf', b'@r1 c\r\nACGT\r\n+\r\n!#!#\r\n@r2\r\nGG\r\n+\r\n##\r\n'),
    ('quality_begins_with_at', b'@r1\nACGT\n+\n@!!!\n@r2\nAC\n+\n@@\n@r3\nA\n+\n@\n'),
    ('plus_line_with_text', b'@r1\nACGT\n+r1 and more\n!!!!\n@r2\nAC\n+@r9\n##\n'),
    ('header_forms', b'@r1 a comment  here\nAC\n+\n!!\n@r2\tx=1\nGT\n+\n##\n@ r3 spaced\nTT\n+\n$$\n@\tr4\nA\n+\n%\n  @r5  \nC\n+\n&\n'),
    ('blanks_of_all_kinds', b'@r1\n \t\x0b\x0cAC GT\r \n+\n\x0c\x0b!! !!\t \r\n@r2 \x0b\x0c\r\n\r\rAC\x0c\n \r+\n\t##\x0b\n'),
    ('lower_case', b'@r1\nacgtnACGTNryk\n+\nabcdefghijklm\n@r2\nzZaA{`@[\n+\n!!!!!!!!\n'),
    ('empty_lines', b'@r1\n\n+\n\n@r2\nA\n+\n!\n@r3\n \t\n+\n\r\n'),
    ('repeated_name', b'@r1\nAAAA\n+\n!!!!\n@r2\nCC\n+\n##\n@r1\nGGG\n+\n$$$\n@r3\nT\n+\n%\n@r2\nTTTTT\n+\n&&&&&\n'),
    ('no_final_newline', b'@r1\nACGT\n+\n!!!!\n@r2\nGG\n+\n##'),
    ('quality_longer_and_shorter', b'@r1\nACGT\n+\n!!!!!!\n@r2\nACGT\n+\n##\n'),
    ('seven_records', b''.join(b'@s%d\n%s\n+\n%s\n' % (k, b'ACGT' * (k + 1), b'!#%&' * (k + 1)) for k in range(7))),
]
HOST = [
    ('blank_line_between_records', b'@r1\nACGT\n+\n!!!!\n\n@r2\nGG\n+\n##\n'),
    ('trailing_blank_line', b'@r1\nACGT\n+\n!!!!\n\n'),
    ('four_trailing_blank_lines', b'@r1\nACGT\n+\n!!!!\n\n\n\n\n'),
    ('three_lines', b'@r1\nACGT\n+\n'),
    ('five_lines', b'@r1\nACGT\n+\n!!!!\n@r2\n'),
    ('six_lines', b'@r1\nACGT\n+\n!!!!\n@r2\nGG\n'),
    ('bare_at', b'@r1\nACGT\n+\n!!!!\n@\nGG\n+\n##\n'),
    ('bare_at_with_blanks', b'@r1\nACGT\n+\n!!!!\n @ \t\nGG\n+\n##\n'),
    ('line_4k_opens_no_record', b'@r1\nAC\n+\n!!\nr2\nGG\n+\n##\n'),
    ('record_opens_off_the_grid', b'@r1\nAC\n+\n!!\nxx\n@r2\nGG\n+\n##\nyy\nzz\nww\n'),
    ('high_byte_in_name', b'@r1\nAC\n+\n!!\n@' + E + b'\nGG\n+\n##\n'),
    ('high_byte_in_sequence', b'@r1\nAC\n+\n!!\n@r2\nG' + E + b'G\n+\n####\n'),
    ('high_byte_in_plus_line', b'@r1\nAC\n+\n!!\n@r2\nGG\n+' + E + b'\n##\n'),
    ('high_byte_in_quality', b'@r1\nAC\n+\n!!\n@r2\nGGGG\n+\n#' + E + b'#\n'),
]


def record(name, text, kind):
    out = io.StringIO()
    entry = dict(name=name, kind=kind, text=base64.b64encode(text).decode('ascii'))
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, 'reads.fastq')
        with open(path, 'wb') as f:
            f.write(text)
        try:
            reads = ref_misc.load_fastq(path, output=out, dot_interval=3)
            entry['items'] = [[k, v[0], v[1]] for k, v in reads.items()]
        except SystemExit as e:
            entry['exit'] = str(e.code)
        except BaseException as e:                         # noqa: BLE001  (what the reference raises is what is recorded)
            entry['exception'] = type(e).__name__
    entry['output'] = out.getvalue()
    return entry


def main():
    doc = dict(reference_version=ref_version.__version__,
               texts=[record(n, t, 'regular') for n, t in REGULAR] + [record(n, t, 'host') for n, t in HOST])
    assert all('items' in e for e in doc['texts'] if e['kind'] == 'regular')
    with gzip.GzipFile(OUT, 'wb', mtime=0) as f:
        f.write(json.dumps(doc, indent=1, sort_keys=True).encode())
    print(OUT, len(doc['texts']), 'texts')
    for e in doc['texts']:
        print(' ', e['name'], e.get('exception') or e.get('exit') or len(e['items']))


if __name__ == '__main__':
    main()
