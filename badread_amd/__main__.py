"""
The `badread` command line for the MI355X path (python -m badread_amd simulate | error_model | qscore_model | plot ...).

Flags, defaults, derived fields, validation messages and exit codes follow the reference CLI
(/root/reference/badread/__main__.py:83-147 flags, :239-336 checks) so that existing command lines and
scripts keep working.  `error_model` and `qscore_model` (the model builders) run their counting
loops on the GPU (badread_amd/model_builder.py), and so does `plot` with its per-base and per-window loops
(badread_amd/plot_window_identity.py; only drawing needs matplotlib).  Additive options: the MI355X group of each command.  Multi-GPU: launch with
`python -m torch.distributed.run --nproc-per-node N -m badread_amd simulate ...`; rank 0 writes stdout.
"""
import argparse
import os
import pathlib
import sys

# A hardware queue per HIP stream of every batch in flight (8 batches x up to 3 streams): HIP's default of 4 queues
# serialises kernels of different streams.  Must be in the environment before the HIP runtime starts (the first torch.cuda
# call), which is why it is set here, at the top of the command line's module, and not where the streams are created.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '32')

from . import settings
from .misc import str_is_dna_sequence, str_is_int
from .version import __version__

ERROR_MODEL_NAMES = ['random', 'nanopore2018', 'nanopore2020', 'nanopore2023', 'pacbio2016', 'pacbio2021']
QSCORE_MODEL_NAMES = ['random', 'ideal', 'nanopore2018', 'nanopore2020', 'nanopore2023', 'pacbio2016', 'pacbio2021']
OUT_OF_SCOPE = ()                        # commands of the reference that are parsed and then refused: none is left

# (group title, group description, [(flag, kwargs), ...]) -- help texts as in the reference
SIMULATE_OPTIONS = [
    ('Required arguments', None, [
        ('--reference', dict(type=str, required=True, help='Reference FASTA file (can be gzipped)')),
        ('--quantity', dict(type=str, required=True,
                            help='Either an absolute value (e.g. 250M) or a relative depth (e.g. 25x)')),
    ]),
    ('Simulation parameters', 'Length and identity and error distributions', [
        ('--length', dict(type=str, default='15000,13000',
                          help='Fragment length distribution (mean and stdev, default: %(default)s)')),
        ('--identity', dict(type=str, default='95,99,2.5',
                            help='Sequencing identity distribution (mean,max,stdev for beta distribution or '
                                 'mean,stdev for normal qscore distribution, default: %(default)s)')),
        ('--error_model', dict(type=str, default='nanopore2023',
                               help='Can be "nanopore2018", "nanopore2020", "nanopore2023", "pacbio2016", '
                                    '"pacbio2021", "random" or a model filename')),
        ('--qscore_model', dict(type=str, default='nanopore2023',
                                help='Can be "nanopore2018", "nanopore2020", "nanopore2023", "pacbio2016", '
                                     '"pacbio2021", "random", "ideal" or a model filename')),
        ('--seed', dict(type=int, help='Random number generator seed for deterministic output (default: '
                                       'different output each time)')),
    ]),
    ('Adapters', 'Controls adapter sequences on the start and end of reads', [
        ('--start_adapter', dict(type=str, default='90,60',
                                 help='Adapter parameters for read starts (rate and amount, default: %(default)s)')),
        ('--end_adapter', dict(type=str, default='50,20',
                               help='Adapter parameters for read ends (rate and amount, default: %(default)s)')),
        ('--start_adapter_seq', dict(type=str, default='AATGTACTTCGTTCAGTTACGTATTGCT',
                                     help='Adapter sequence for read starts')),
        ('--end_adapter_seq', dict(type=str, default='GCAATACGTAACTGAACGAAGT', help='Adapter sequence for read ends')),
    ]),
    ('Problems', 'Ways reads can go wrong', [
        ('--junk_reads', dict(type=float, default=1, help='This percentage of reads will be low-complexity junk')),
        ('--random_reads', dict(type=float, default=1, help='This percentage of reads will be random sequence')),
        ('--chimeras', dict(type=float, default=1, help='Percentage at which separate fragments join together')),
        ('--glitches', dict(type=str, default='10000,25,25',
                            help='Read glitch parameters (rate, size and skip, default: %(default)s)')),
        ('--small_plasmid_bias', dict(action='store_true',
                                      help='If set, then small circular plasmids are lost when the fragment length is '
                                           'too high (default: small plasmids are included regardless of fragment '
                                           'length)')),
    ]),
    ('MI355X', 'Device options (additive; no effect on the simulated reads)', [
        ('--gpu-batch', dict(type=int, default=None, dest='gpu_batch',
                             help='Maximum reads per device batch and GPU (default: 65536)')),
        ('--gzip', dict(type=int, default=None, dest='gzip_level', metavar='LEVEL',
                        help='Write gzip-compressed FASTQ to stdout, compressed on all host cores (level 0-9); '
                             'default: plain text, as the reference')),
        ('--gzip-device', dict(action='store_true', dest='gzip_device',
                               help='Write gzip-compressed FASTQ to stdout, compressed on the GPU before the bytes cross PCIe '
                                    '(a Huffman code per sequence line and per quality line, no match search: smaller than '
                                    'gzip -6 on simulated reads, and the host only copies)')),
        ('--output-shards', dict(type=str, default=None, dest='output_shards', metavar='PREFIX',
                                 help='Multi-GPU runs: every rank writes the records of ITS reads to PREFIX.<rank>.fastq (.fastq.gz with '
                                      '--gzip / --gzip-device) and the bytes per batch to PREFIX.<rank>.parts (FASTQ text bytes; with '
                                      '--gzip-device the compressed bytes; with --gzip the compressed bytes per batch go to '
                                      'PREFIX.<rank>.zparts beside them), instead of all records travelling to rank 0 and through one '
                                      'stdout; the same reads, the same stopping point')),
        ('--truth-paf', dict(type=str, default=None, dest='truth_paf', metavar='PATH',
                             help='Also write the true alignment of every read against the reference to PATH as PAF (plain text): '
                                  'one record per stretch of the read that comes consecutively from one contig and strand, with a '
                                  'cg:Z: CIGAR; with --output-shards every rank writes PATH.<rank>')),
        ('--truth-sam', dict(type=str, default=None, dest='truth_sam', metavar='PATH',
                             help='Also write the same true alignments to PATH as SAM (plain text, with header): one line per PAF '
                                  'record, the whole read with SEQ, QUAL and the FASTQ header (CO:Z:) on the primary line, the '
                                  'record\'s slice on the supplementary ones, one unmapped line for a read with no record; can be '
                                  'combined with --truth-paf; with --output-shards every rank writes PATH.<rank>')),
        ('--truth-bam', dict(type=str, default=None, dest='truth_bam', metavar='PATH',
                             help='Also write the same true alignments to PATH as BAM (BGZF-compressed on the GPU): the header '
                                  'and the records of --truth-sam, in the same order, unsorted; can be combined with --truth-paf '
                                  'and --truth-sam; with --output-shards every rank writes PATH.<rank>, a complete BAM file')),
        ('--truth-bam-sorted', dict(type=str, default=None, dest='truth_bam_sorted', metavar='PATH',
                                    help='Also write the records of --truth-bam to PATH in coordinate order (sorted on the GPU when the '
                                         'job has ended, unmapped records last, SO:coordinate) and their BAI index to PATH.bai: no '
                                         'samtools sort or index needed; takes --truth-tags, --truth-cs and --truth-eqx; works alone '
                                         'or with the other truth files; with --output-shards every rank writes PATH.<rank> and '
                                         'PATH.<rank>.bai for its own reads')),
        ('--truth-tags', dict(type=str, default=None, dest='truth_tags', metavar='LIST',
                              help='Tags to add to the records of --truth-sam and --truth-bam, a comma-separated list of MD and SA: '
                                   'MD:Z: (mismatched and deleted reference bases) on every mapped line, SA:Z: (the read\'s other '
                                   'alignments) on every mapped line of a read with two or more')),
        ('--truth-cs', dict(type=str, default=None, dest='truth_cs', metavar='MODE',
                            help='Add minimap2\'s cs:Z: tag to every record of --truth-paf and every mapped line of --truth-sam and '
                                 '--truth-bam: short (:n for matching stretches) or long (=ACGT, the matching bases spelt out)')),
        ('--truth-eqx', dict(action='store_true', default=False, dest='truth_eqx',
                             help='Write the CIGARs of --truth-paf, --truth-sam and --truth-bam with = and X in place of M '
                                  '(such a PAF is not input for error_model / qscore_model)')),
        ('--truth-depth', dict(type=str, default=None, dest='truth_depth', metavar='PATH',
                               help='Also write the true coverage of the reference to PATH as bedGraph (plain text, no header): '
                                    'contig, start, end (0-based, half-open) and the number of true alignments over every base, '
                                    'zero-depth stretches included; works alone or with the other truth files; with '
                                    '--output-shards every rank writes PATH.<rank>, the coverage by its own reads')),
        ('--gpu-streams', dict(type=int, default=None, dest='gpu_streams',
                               help='Device batches in flight per GPU, each on its own HIP stream (default: 6)')),
    ]),
]


class _Parser(argparse.ArgumentParser):
    """Usage errors print the help and exit with status 2, like the reference's parser."""

    def error(self, message):
        self.print_help(file=sys.stderr)
        sys.exit(2)


def _add_help_group(parser):
    other = parser.add_argument_group('Other' if parser.prog.endswith('simulate') else 'Help')
    other.add_argument('-h', '--help', action='help', default=argparse.SUPPRESS, help='Show this help message and exit')
    other.add_argument('--version', action='version', version='Badread v' + __version__,
                       help="Show program's version number and exit")


def parse_args(argv):
    parser = _Parser(prog='badread', add_help=False,
                     description='Badread: a long read simulator that can imitate many types of read problems '
                                 '(MI355X-native simulate path)')
    subparsers = parser.add_subparsers(title='Commands', dest='subparser_name')
    sim = subparsers.add_parser('simulate', description='Generate fake long reads', add_help=False)
    for title, description, options in SIMULATE_OPTIONS:
        group = sim.add_argument_group(title, description=description)
        for flag, kwargs in options:
            group.add_argument(flag, **kwargs)
    _add_help_group(sim)
    # the model builders: flags and defaults of the reference (__main__.py:150-205)
    em = subparsers.add_parser('error_model', description='Build a Badread error model', add_help=False)
    qm = subparsers.add_parser('qscore_model', description='Build a Badread qscore model', add_help=False)
    for sub in (em, qm):
        req = sub.add_argument_group('Required arguments')
        req.add_argument('--reference', type=str, required=True, help='Reference FASTA file')
        req.add_argument('--reads', type=str, required=True, help='FASTQ of real reads')
        req.add_argument('--alignment', type=str, required=True, help='PAF alignment of reads aligned to reference')
    opt = em.add_argument_group('Optional arguments')
    opt.add_argument('--k_size', type=int, default=7, help='Error model k-mer size')
    opt.add_argument('--max_alignments', type=int, help='Only use this many alignments when generating error model '
                                                        '(default: use all alignments)')
    opt.add_argument('--max_alt', type=int, default=25, help='Only save up to this many alternatives to each k-mer')
    opt = qm.add_argument_group('Optional arguments')
    opt.add_argument('--k_size', type=int, default=9, help='Qscore model k-mer size (must be odd, default: %(default)s)')
    opt.add_argument('--max_alignments', type=int, help='Only use this many alignments when generating qscore model '
                                                        '(default: use all alignments)')
    opt.add_argument('--max_del', type=int, default=6, help='Deletion runs longer than this will be collapsed to reduce '
                                                            'the number of possible alignments')
    opt.add_argument('--min_occur', type=int, default=100, help='CIGARs which occur less than this many times will not be '
                                                                'included in the model')
    opt.add_argument('--max_output', type=int, default=10000, help='The outputted model will be limited to this many lines')
    loader = dict(action='store_true', dest='gpu_loader', help='Parse the PAF\'s CIGARs and pack the alignments on the GPU (same output)')
    reads = dict(action='store_true', dest='gpu_reads', help='Parse the FASTQ and pack the read slices on the GPU (same output; needs --gpu-loader)')
    for sub in (em, qm):
        group = sub.add_argument_group('MI355X', description='Additive options (no effect on the model)')
        group.add_argument('--gpu-loader', **loader)
        group.add_argument('--gpu-reads', **reads)
    _add_help_group(em)
    _add_help_group(qm)
    # plot: flags and defaults of the reference (__main__.py:208-228) and a group of additive ones
    pl = subparsers.add_parser('plot', description='View read identities over a sliding window', add_help=False)
    req = pl.add_argument_group('Required arguments')
    req.add_argument('--reference', type=str, required=True, help='Reference FASTA file')
    req.add_argument('--reads', type=str, required=True, help='FASTQ of real reads')
    req.add_argument('--alignment', type=str, required=True, help='PAF alignment of reads aligned to reference')
    opt = pl.add_argument_group('Optional arguments')
    opt.add_argument('--window', type=int, default=100, help='Window size in bp')
    opt.add_argument('--qual', action='store_true', help='Include qscores in plot (default: only show identity)')
    opt.add_argument('--no_plot', action='store_true', help='Do not display plots (for testing purposes)')
    gpu = pl.add_argument_group('MI355X', description='Additive options (no effect on the numbers)')
    gpu.add_argument('--summary', type=str, default=None, metavar='PATH',
                     help='Write one TSV line per alignment to PATH: the alignment, its number of windows, the lowest window '
                          'identity and where it is, the highest and the mean (with --qual the same of the window qualities)')
    gpu.add_argument('--save', type=str, default=None, metavar='DIR',
                     help='Save one PNG per alignment to DIR/<index>_<read name>.png instead of displaying it')
    gpu.add_argument('--max_alignments', type=int, help='Only use this many alignments of the PAF (default: use all alignments)')
    gpu.add_argument('--gpu-loader', **loader)
    gpu.add_argument('--gpu-reads', **reads)
    _add_help_group(pl)
    for name in OUT_OF_SCOPE:
        sub = subparsers.add_parser(name, add_help=False, description=f'{name}: not part of the MI355X build')
        sub.add_argument('rest', nargs=argparse.REMAINDER)
    _add_help_group(parser)
    if len(argv) == 0:
        parser.print_help(file=sys.stderr)
        sys.exit(1)
    return parser.parse_args(argv)


def _floats(text, count=None):
    values = [float(x) for x in text.split(',')]
    if count is not None and len(values) < count:
        raise IndexError(text)
    return values


TRUTH_TAGS = {'MD': 1, 'SA': 2}          # include/brx.h: BRX_TAG_MD, BRX_TAG_SA


def truth_tags_mask(text, has_file):
    """--truth-tags LIST as the bit mask simulate() reads (0 without the option)."""
    if text is None:
        return 0
    parts = text.split(',')
    if not all(x in TRUTH_TAGS for x in parts):
        sys.exit('Error: --truth-tags must be a comma-separated list of MD and SA')
    if not has_file:
        sys.exit('Error: --truth-tags needs --truth-sam or --truth-bam')
    return sum({TRUTH_TAGS[x] for x in parts})


FMT_EQX, FMT_CS, FMT_CS_LONG = 1, 2, 4   # include/brx.h: BRX_FMT_EQX, BRX_FMT_CS, BRX_FMT_CS_LONG


def truth_fmt_mask(cs, eqx, has_file):
    """--truth-cs MODE and --truth-eqx as the bit mask simulate() reads (0 without the options)."""
    if cs is not None and cs not in ('short', 'long'):
        sys.exit('Error: --truth-cs must be short or long')
    for on, flag in ((cs is not None, '--truth-cs'), (eqx, '--truth-eqx')):
        if on and not has_file:
            sys.exit(f'Error: {flag} needs --truth-paf, --truth-sam or --truth-bam')
    return (FMT_EQX if eqx else 0) | (0 if cs is None else FMT_CS if cs == 'short' else FMT_CS | FMT_CS_LONG)


def check_simulate_args(args):
    """Validate and derive the fields simulate() reads (mean_frag_length, identity triple, glitch_*)."""
    if not pathlib.Path(args.reference).is_file():
        sys.exit(f'Error: {args.reference} is not a file')
    for flag in ('truth_paf', 'truth_sam', 'truth_bam', 'truth_bam_sorted', 'truth_depth'):
        path = getattr(args, flag, None)
        if path is not None and not pathlib.Path(path).resolve().parent.is_dir():
            sys.exit(f'Error: the directory of --{flag.replace("_", "-")} {path} does not exist')
    # --truth-bam-sorted is a file of records like --truth-bam: the tags and the formats go into it
    bam = getattr(args, 'truth_bam', None) or getattr(args, 'truth_bam_sorted', None)
    args.truth_tags = truth_tags_mask(getattr(args, 'truth_tags', None), getattr(args, 'truth_sam', None) or bam)
    args.truth_fmt = truth_fmt_mask(getattr(args, 'truth_cs', None), bool(getattr(args, 'truth_eqx', False)),
                                    bool(bam) or any(getattr(args, flag, None) for flag in ('truth_paf', 'truth_sam')))
    for value, names, flag in ((args.error_model, ERROR_MODEL_NAMES, '--error_model'),
                               (args.qscore_model, QSCORE_MODEL_NAMES, '--qscore_model')):
        if value.lower() not in names and not pathlib.Path(value).is_file():
            sys.exit(f'Error: {value} is not a file\n  {flag} must be from {names} or a filename')

    for limit_hit, message in ((args.chimeras > 50, '--chimeras cannot be greater than 50'),
                               (args.junk_reads > 100, '--junk_reads cannot be greater than 100'),
                               (args.random_reads > 100, '--random_reads cannot be greater than 100'),
                               (args.junk_reads + args.random_reads > 100,
                                '--junk_reads and --random_reads cannot sum to more than 100')):
        if limit_hit:
            sys.exit('Error: ' + message)

    try:
        args.mean_frag_length, args.frag_length_stdev = _floats(args.length, 2)[:2]
    except (ValueError, IndexError):
        sys.exit('Error: could not parse --length values')
    if args.mean_frag_length <= settings.MIN_MEAN_READ_LENGTH:
        sys.exit(f'Error: mean read length must be at least {settings.MIN_MEAN_READ_LENGTH}')
    if args.frag_length_stdev < 0:
        sys.exit('Error: read length stdev cannot be negative')

    try:
        identity = _floats(args.identity)
    except ValueError:
        sys.exit('Error: could not parse --identity values')
    if len(identity) == 2:
        args.mean_identity, args.max_identity, args.identity_stdev = identity[0], None, identity[1]
        check_qscore_identities(args)
    elif len(identity) == 3:
        args.mean_identity, args.max_identity, args.identity_stdev = identity
        check_beta_identities(args)
    else:
        sys.exit('Error: could not parse --identity values')

    try:
        args.glitch_rate, args.glitch_size, args.glitch_skip = _floats(args.glitches, 3)[:3]
    except (ValueError, IndexError):
        sys.exit('Error: could not parse --glitches values')
    if min(args.glitch_rate, args.glitch_size, args.glitch_skip) < 0:
        sys.exit('Error: --glitches must contain non-negative values')

    for attr, flag in (('start_adapter_seq', '--start_adapter_seq'), ('end_adapter_seq', '--end_adapter_seq')):
        value = getattr(args, attr)
        if value != '' and not str_is_int(value):
            value = value.upper()
            setattr(args, attr, value)
            if not str_is_dna_sequence(value):
                sys.exit(f'Error: {flag} must be a DNA sequence or a number')


def check_beta_identities(args):
    floor = settings.MIN_MEAN_READ_IDENTITY
    checks = ((args.mean_identity > 100.0, 'mean read identity cannot be more than 100'),
              (args.max_identity > 100.0, 'max read identity cannot be more than 100'),
              (args.mean_identity <= floor, f'mean read identity must be at least {floor}'),
              (args.max_identity <= floor, f'max read identity must be at least {floor}'),
              (args.mean_identity > args.max_identity,
               f'mean identity ({args.mean_identity}) cannot be larger than max identity ({args.max_identity})'),
              (args.identity_stdev < 0.0, 'read identity stdev cannot be negative'))
    for failed, message in checks:
        if failed:
            sys.exit('Error: ' + message)


def check_qscore_identities(args):
    if args.mean_identity <= settings.MIN_MEAN_READ_QSCORE:
        sys.exit(f'Error: mean read identity must be at least {settings.MIN_MEAN_READ_QSCORE}')
    if args.identity_stdev < 0.0:
        sys.exit('Error: read qscore stdev cannot be negative')


def check_python_version():
    if sys.version_info.major < 3 or sys.version_info.minor < 6:
        sys.exit('Error: Badread requires Python 3.6 or later')


def main(output=sys.stderr):
    check_python_version()
    args = parse_args(sys.argv[1:])
    if args.subparser_name == 'simulate':
        check_simulate_args(args)
        from . import simulate as sim
        if args.gpu_batch:
            sim.DEFAULT_MAX_BATCH = int(args.gpu_batch)
        sim.simulate(args, output=output)
    elif args.subparser_name == 'error_model':
        from .model_builder import make_error_model
        make_error_model(args, output=output)
    elif args.subparser_name == 'qscore_model':
        from .model_builder import make_qscore_model
        make_qscore_model(args, output=output)
    elif args.subparser_name == 'plot':
        from .plot_window_identity import plot_window_identity
        plot_window_identity(args)
    elif args.subparser_name in OUT_OF_SCOPE:
        sys.exit(f'Error: the {args.subparser_name} command is not part of the MI355X simulate build; '
                 f'use the reference Badread for it')
    else:
        parse_args([])


if __name__ == '__main__':
    main()
