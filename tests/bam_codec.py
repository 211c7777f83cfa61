"""
TEST INFRASTRUCTURE: BAM and BGZF in plain Python (struct + gzip + zlib), for the --truth-bam tests.  No tool that reads BAM is
assumed to be installed, so the decoder is part of the tests.

`bam_from` restates the contract of brx_emit_bam (README, --truth-bam): the BAM records of the lines of a --truth-sam file.
`sam_of_bam` is written independently of it: a general decoder of uncompressed BAM records back to SAM text, which reads a
CG:B:I tag back into the CIGAR.  `bgzf_blocks` walks a BGZF file block by block and checks every block's framing.
"""
import re
import struct
import zlib

SEQ_SET = '=ACMGRSVTWYHKDBN'
CIGAR_OPS = 'MIDNSH'
_CIGAR = re.compile(r'(\d+)([MIDNSH])')


# ---------------------------------------------------------------------------------------------
# SAM lines -> BAM records (the contract)
# ---------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """SAM spec v1 section 5.3, for [beg, end)."""
    end -= 1
    for shift, levels in ((14, 15), (17, 12), (20, 9), (23, 6), (26, 3)):
        if beg >> shift == end >> shift:
            return ((1 << levels) - 1) // 7 + (beg >> shift)
    return 0


def int_tag(tag, value):
    """An integer tag in the smallest type that holds it (htslib's rule)."""
    if value >= 0:
        kind = ('C', 'B') if value <= 255 else ('S', 'H') if value <= 65535 else ('I', 'I')
    else:
        kind = ('c', 'b') if value >= -128 else ('s', 'h') if value >= -32768 else ('i', 'i')
    return tag.encode() + kind[0].encode() + struct.pack('<' + kind[1], value)


def bam_from(sam_records, contig_names, max_cigar_ops=65535):
    """The uncompressed BAM records of the record lines (no header) of a --truth-sam file, back to back."""
    ref_id = {name: i for i, name in enumerate(contig_names)}
    out = []
    for line in bytes(sam_records).decode('latin-1').splitlines():
        f = line.split('\t')
        name, flag, seq, qual = f[0], int(f[1]), f[9], f[10]
        assert len(name) == 36 and f[6:9] == ['*', '0', '0']
        ops = [(int(n), CIGAR_OPS.index(x)) for n, x in _CIGAR.findall(f[5])] if f[5] != '*' else []
        reflen = sum(n for n, x in ops if x in (0, 2))
        if flag & 4:
            rid, pos, mapq, bin_ = -1, -1, 0, 4680
        else:
            rid, pos, mapq = ref_id[f[2]], int(f[3]) - 1, int(f[4])
            bin_ = reg2bin(pos, pos + reflen) & 0xFFFF
        tags = b''
        for t in f[11:]:
            if t[2:5] == ':i:':
                tags += int_tag(t[:2], int(t[5:]))
            else:
                assert t[2:5] == ':Z:'
                tags += t[:2].encode() + b'Z' + t[5:].encode('latin-1') + b'\0'
        cigar = ops
        if len(ops) > max_cigar_ops:
            cigar = [(len(seq), 4), (reflen, 3)]
            tags += b'CGBI' + struct.pack('<I', len(ops)) + b''.join(struct.pack('<I', n << 4 | x) for n, x in ops)
        nib = [SEQ_SET.index(c) if c in SEQ_SET else 15 for c in seq.upper()] + [0]
        packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
        body = struct.pack('<iiBBHHHIiii', rid, pos, len(name) + 1, mapq, bin_, len(cigar), flag, len(seq), -1, -1, 0)
        body += name.encode() + b'\0' + b''.join(struct.pack('<I', n << 4 | x) for n, x in cigar)
        body += packed + bytes(ord(c) - 33 for c in qual) + tags
        out.append(struct.pack('<I', len(body)) + body)
    return b''.join(out)


# ---------------------------------------------------------------------------------------------
# BAM records -> SAM lines (an independent decoder)
# ---------------------------------------------------------------------------------------------
_SCALAR = {'A': ('c', 1), 'c': ('b', 1), 'C': ('B', 1), 's': ('h', 2), 'S': ('H', 2), 'i': ('i', 4), 'I': ('I', 4), 'f': ('f', 4)}


def _tags(raw, at, end):
    """[(tag, type, value)] of the tag bytes raw[at:end]."""
    tags = []
    while at < end:
        tag, kind = raw[at:at + 2].decode(), chr(raw[at + 2])
        at += 3
        if kind == 'Z':
            stop = raw.index(b'\0', at)
            tags.append((tag, 'Z', raw[at:stop].decode('latin-1')))
            at = stop + 1
        elif kind == 'B':
            sub, count = chr(raw[at]), struct.unpack_from('<I', raw, at + 1)[0]
            fmt, size = _SCALAR[sub]
            tags.append((tag, 'B' + sub, list(struct.unpack_from(f'<{count}{fmt}', raw, at + 5))))
            at += 5 + count * size
        else:
            fmt, size = _SCALAR[kind]
            tags.append((tag, kind, struct.unpack_from('<' + fmt, raw, at)[0]))
            at += size
    assert at == end
    return tags


def records_of_bam(raw):
    """The records of uncompressed BAM record bytes as dicts of their decoded fields (the CIGAR as it is stored)."""
    raw, at, out = bytes(raw), 0, []
    while at < len(raw):
        size = struct.unpack_from('<I', raw, at)[0]
        end = at + 4 + size
        assert end <= len(raw)
        rid, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_rid, next_pos, tlen = struct.unpack_from('<iiBBHHHIiii', raw, at + 4)
        p = at + 36
        name = raw[p:p + l_name]
        assert name[-1:] == b'\0'
        p += l_name
        cigar = [(w >> 4, w & 15) for w in struct.unpack_from(f'<{n_cigar}I', raw, p)]
        p += 4 * n_cigar
        packed = raw[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = ''.join(SEQ_SET[b >> 4] + SEQ_SET[b & 15] for b in packed)[:l_seq]
        assert l_seq % 2 == 0 or packed[-1] & 15 == 0              # the spare nibble of an odd SEQ is 0
        qual = raw[p:p + l_seq]
        p += l_seq
        out.append(dict(rid=rid, pos=pos, mapq=mapq, bin=bin_, flag=flag, l_seq=l_seq, next=(next_rid, next_pos, tlen), name=name[:-1].decode(),
                        cigar=cigar, seq=seq, qual=qual, tags=_tags(raw, p, end)))
        at = end
    return out


def sam_of_bam(raw, contig_names):
    """The SAM text of uncompressed BAM record bytes; a CG:B:I tag behind a `kSmN` CIGAR is read back into the CIGAR."""
    lines = []
    for r in records_of_bam(raw):
        cigar, tags = r['cigar'], r['tags']
        cg = [t for t in tags if t[0] == 'CG']
        if cg:
            assert cg[0][1] == 'BI' and tags[-1] is cg[0] and len(cigar) == 2 and cigar[0] == (r['l_seq'], 4) and cigar[1][1] == 3
            cigar, tags = [(w >> 4, w & 15) for w in cg[0][2]], tags[:-1]
        text = ''.join(f'{n}{CIGAR_OPS[x]}' for n, x in cigar) or '*'
        nxt = ['*' if r['next'][0] < 0 else contig_names[r['next'][0]], str(r['next'][1] + 1), str(r['next'][2])]
        fields = [r['name'], str(r['flag']), '*' if r['rid'] < 0 else contig_names[r['rid']], str(r['pos'] + 1), str(r['mapq']), text] + nxt
        fields += [r['seq'], ''.join(chr(q + 33) for q in r['qual'])]
        fields += [f'{t}:{"Z" if k == "Z" else "i"}:{v}' for t, k, v in tags]
        lines.append('\t'.join(fields) + '\n')
    return ''.join(lines).encode('latin-1')


# ---------------------------------------------------------------------------------------------
# BGZF
# ---------------------------------------------------------------------------------------------
def bgzf_blocks(blob):
    """The payloads of the BGZF blocks of `blob`, every block's framing checked: the gzip magic with FEXTRA, the BC subfield, BSIZE + 1
    = the block's real size <= 65536, ISIZE <= 65536; inflated as a gzip member, so that CRC-32 and length are verified."""
    blob, at, payloads = bytes(blob), 0, []
    while at < len(blob):
        assert blob[at:at + 4] == b'\x1f\x8b\x08\x04', (at, blob[at:at + 4])
        xlen = struct.unpack_from('<H', blob, at + 10)[0]
        assert xlen == 6 and blob[at + 12:at + 16] == b'BC\x02\x00', (at, blob[at + 10:at + 18])
        size = struct.unpack_from('<H', blob, at + 16)[0] + 1
        assert size <= 65536 and at + size <= len(blob)
        member = zlib.decompressobj(31)
        payload = member.decompress(blob[at:at + size])
        assert member.eof and member.unused_data == b'', at            # the member ends exactly where BSIZE says
        assert len(payload) <= 65536 and struct.unpack_from('<I', blob, at + size - 4)[0] == len(payload)
        payloads.append(payload)
        at += size
    return payloads
