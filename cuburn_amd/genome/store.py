"""
Where genomes come from: a directory of ``<id>.json`` files, one JSON document holding many
genomes (``{"type": "onefiledb", id: genome, ...}``), or a flam3 XML file named directly.

One class; it offers the ``get(id)`` that edge blending uses to follow an edge's links to its
nodes (cuburn/genome/blend.py), plus ``animation(name)`` for callers that want something
renderable whatever the stored type is.
"""
import copy
import json
import os
import warnings

_XML_EXT = ('.flam3', '.flame')


class GenomeStore(object):
    def __init__(self, path='.'):
        self.path = path
        self.docs = {}                  # ids held in memory: the one-file document, or stashed genomes
        self.directory = None
        if os.path.isdir(path):
            self.directory = path
        else:
            with open(path) as fp:
                doc = json.load(fp)
            if not isinstance(doc, dict) or doc.get('type') != 'onefiledb':
                raise ValueError('%s is neither a directory nor a onefiledb document' % path)
            self.docs.update((k, v) for k, v in doc.items() if k != 'type')

    def stash(self, ident, genome):
        self.docs[ident] = genome

    def get(self, ident):
        if ident in self.docs:
            return self.docs[ident]
        if self.directory is None:
            raise KeyError(ident)
        fn = ident if ident.endswith('.json') else ident + '.json'
        with open(os.path.join(self.directory, fn)) as fp:
            return json.load(fp)

    def animation(self, name, half=False):
        """``(animation genome, basename for output files)`` for an id or a flam3 XML path."""
        from . import convert
        stem, ext = os.path.splitext(os.path.basename(name))
        if ext in _XML_EXT and os.path.isfile(name):
            with open(name) as fp:
                flames = convert.XMLGenomeParser.parse(fp.read())
            if len(flames) != 1:
                warnings.warn('%d flames in file, only using one.' % len(flames))
            genome = convert.flam3_to_node(flames[0])
        else:
            genome = self.get(name)
            if ext not in _XML_EXT + ('.json',):
                stem = os.path.basename(name)
        kind = genome.get('type')
        if kind == 'node':
            # `chaos` (flam3 xaos) is an animation-only key (genome/specs.py): it is taken off the node, and put onto the loop of
            # the node against itself, whose xform `k` is `k_k` (natural sort)
            genome, tables = _take_chaos(genome)
            genome = convert.node_to_anim(_NoChaos(self), genome, half=half)
            _put_chaos(genome, tables)
        elif kind == 'edge':
            genome, tables = _take_chaos(genome)
            if tables:
                warnings.warn('chaos is dropped from edges: blending two xaos tables is not defined', UserWarning, stacklevel=2)
            genome = convert.edge_to_anim(_NoChaos(self), genome)
        elif kind != 'animation':
            raise ValueError('unrecognised genome type %r' % kind)
        return genome, stem


def _xform_dicts(genome):
    """(path, xform dict) of every xform of a node or edge: 'xforms.<k>', 'xforms.src.<k>', 'final_xform'."""
    xfs = genome.get('xforms', {})
    if genome.get('type') == 'edge':
        groups = [('xforms.' + side, xfs.get(side, {})) for side in ('src', 'dst')]
    else:
        groups = [('xforms', xfs)]
    out = [(base + '.' + str(k), xf) for base, grp in groups if isinstance(grp, dict) for k, xf in grp.items()]
    out.append(('final_xform', genome.get('final_xform')))
    return [(p, xf) for p, xf in out if isinstance(xf, dict)]


def _take_chaos(genome):
    """A copy of a node or edge without its `chaos` tables, and the tables by xform path."""
    tables = dict((p, xf['chaos']) for p, xf in _xform_dicts(genome) if 'chaos' in xf)
    if not tables:
        return genome, tables
    genome = copy.deepcopy(genome)
    for _, xf in _xform_dicts(genome):
        xf.pop('chaos', None)
    return genome, tables


def _put_chaos(anim, tables):
    """Tables of a node onto the animation of that node against itself: xform `k` -> `k_k`, target `n` -> `n_n`.  Only where
    every xform of the node became `k_k` (what the natural sort of a node against itself gives); otherwise dropped, loudly."""
    if not tables:
        return
    xfs = anim.get('xforms', {})
    keys = set(str(n) for p, t in tables.items() if p != 'final_xform' for n in t) | set(
        p.split('.', 1)[1] for p in tables if p != 'final_xform')
    if not all('%s_%s' % (k, k) in xfs for k in keys):
        warnings.warn('chaos is dropped: the xforms of the node did not pair with themselves', UserWarning, stacklevel=3)
        return
    for p, t in tables.items():
        tab = dict(('%s_%s' % (n, n), v) for n, v in t.items())
        if p == 'final_xform':
            anim['final_xform']['chaos'] = tab
        else:
            k = p.split('.', 1)[1]
            xfs['%s_%s' % (k, k)]['chaos'] = tab


class _NoChaos(object):
    """The store as the blender sees it: nodes it fetches (bases, an edge's ends) come without `chaos`."""

    def __init__(self, store):
        self.store = store

    def get(self, ident):
        genome, tables = _take_chaos(self.store.get(ident))
        if tables:
            warnings.warn('chaos of %r is dropped: blending xaos tables is not defined' % ident, UserWarning, stacklevel=2)
        return genome


def connect(path):
    return GenomeStore(path)
