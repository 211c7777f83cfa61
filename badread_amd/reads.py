"""
--gpu-reads (README: The device read loader): the FASTQ of `error_model`, `qscore_model` and `plot` parsed by brx_fastq_scan
(include/brx.h; kernels in csrc/brx_fastqin.h) and left on the device, where brx_reads_pack cuts the read slices of a job out of it
(model_builder.Job.packed).  The host reads the file, uploads it and touches a record once, for its name.

load_fastq_device stands in for misc.load_fastq: the same mapping, the same text on `output`, the same exits.  A file that is not of
the regular layout (include/brx.h: blank lines, a record cut short, a line 4k that opens no record, a byte of 0x80 or more) is loaded
by misc.load_fastq itself, which gives the reference's result or its exception.
"""
import sys

import numpy as np

from .alignment import _out_of_memory
from .misc import get_open_func, get_sequence_file_type, load_fastq


class DeviceReads(object):
    """What load_fastq_device returns: the dict of load_fastq where the commands need one.  text: the file's bytes on the engine's
    device; rec: one record per read in file order (engine.FASTQ_REC_DTYPE); data: the same bytes on the host, from which a read's
    strings are made only when somebody asks (the spill paths of the model builders).  A repeated name keeps its last record, as the
    dict does."""

    def __init__(self, engine, text, rec, data):
        self.engine, self.text, self.rec, self.data = engine, text, rec, data
        at = (rec['head_off'] + rec['name_off']).tolist()
        self.index = {data[o:o + n].decode('ascii'): k for k, (o, n) in enumerate(zip(at, rec['name_len'].tolist()))}
        self._spans = (rec['seq_off'].tolist(), rec['seq_len'].tolist(), rec['qual_off'].tolist(), rec['qual_len'].tolist())

    def __contains__(self, name):
        return name in self.index

    def __len__(self):
        return len(self.index)

    def __iter__(self):
        return iter(self.index)

    def keys(self):
        return self.index.keys()

    def spans(self, name):
        """(where the bases begin in the text, how many, where the qualities begin, how many)"""
        k = self.index[name]
        return tuple(x[k] for x in self._spans)

    def length(self, name):
        """len(self[name][0]) without making the string"""
        return self._spans[1][self.index[name]]

    def __getitem__(self, name):
        seq_at, seq_n, qual_at, qual_n = self.spans(name)
        return self.data[seq_at:seq_at + seq_n].upper().decode('ascii'), self.data[qual_at:qual_at + qual_n].decode('ascii')


def read_length(reads, name):
    """len(reads[name][0]) of either kind of reads"""
    return reads.length(name) if isinstance(reads, DeviceReads) else len(reads[name][0])


def _does_not_fit(engine, n_bytes):
    need = n_bytes + engine.lib.brx_fastq_scan_scratch(n_bytes) + 48 * (n_bytes // 1024 + 64)
    sys.exit(f'Error: --gpu-reads: the read file needs {need / 1e9:.1f} GB on the device')


def load_fastq_device(filename, engine, output=sys.stderr, dot_interval=1000):
    """load_fastq with the per-byte work on the device.  Nothing is printed before the layout is known, so that a file the host has to
    load prints what load_fastq prints and nothing else."""
    if get_sequence_file_type(filename) != 'FASTQ':
        sys.exit('Error: {} is not FASTQ format'.format(filename))
    with get_open_func(filename)(filename, 'rb') as handle:
        data = handle.read()
    try:
        text = engine._upload(np.frombuffer(data, dtype=np.uint8))[1][:len(data)]
        rec, layout = engine.fastq_scan(text)
    except _out_of_memory(engine):
        _does_not_fit(engine, len(data))
    if layout != 0:
        del text
        return load_fastq(filename, output, dot_interval)
    print('Loading reads', end='', file=output, flush=True)
    print('.' * (len(rec) // dot_interval), end='', file=output, flush=True)
    print('', file=output, flush=True)
    return DeviceReads(engine, text, rec, data)
