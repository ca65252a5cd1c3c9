"""
Output modules: pixel-format conversion on device, copy to host, encode.

Role of cuburn/output.py:21-136,411-434: 8-bit RGBA (jpeg / png / raw) and 16-bit RGBA (tiff /
raw16) stills here, on the host or encoded on the device; the outputs that pipe frames into a
video encoder (x264, vpxenc, ffmpeg) are in encoders.py.
"""
import io
import struct
import zlib
import numpy as np

from . import _lib
from .filters import RESIZE_MAX_RATIO       # the widest Lanczos tables the library serves: a proxy's largest step


def _bool(key, v):
    if not isinstance(v, bool):
        raise ValueError('output.%s must be true or false' % key)
    return v


def _int_in(key, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError('output.%s must be an integer in %d..%d' % (key, lo, hi))
    return v


def _one_of(key, v, table, wording):
    if not isinstance(v, str) or v not in table:
        raise ValueError('output.%s must be %s, not "%s"' % (key, wording, v))
    return v


def _bits(v, name='output.bits'):
    if isinstance(v, bool) or not isinstance(v, int) or v not in (8, 16):
        raise ValueError('%s must be 8 or 16' % name)
    return v


class Output(object):
    fmt = 0
    dtype = 'u1'
    suffix = '.raw'

    def convert(self, fb, gprof, dim, stream=None):
        """Conversion and copy are one call here; kept for interface parity (output.py:29-37)."""

    def shape(self, dim):
        """Shape of the host frame ``copy`` returns."""
        return (dim.h, dim.w, 4)

    def copy(self, fb, dim, pool=None, stream=None, dev_out=0, host=True):
        """Queue dither+convert and the async D2H; returns the host array (output.py:85-88).
        ``dev_out``: device address that receives the converted frame instead of the context's own
        pixel buffer (e.g. a tensor that RCCL gathers: no host round trip); ``host=False`` skips the
        D2H copy altogether (returns None)."""
        h_out = fb.host_buffer(self.shape(dim), self.dtype) if host else None
        _lib.check(_lib.load().fl_output(fb.ctx, dim.w, dim.h, self.fmt, h_out.ctypes.data if host else None, int(dev_out)))
        return h_out

    def encode(self, buf):
        if buf is None:
            return {}, []
        return {self.suffix: io.BytesIO(np.ascontiguousarray(buf).tobytes())}, []

    def abort(self):
        """Drop whatever a half-written output holds (encoder processes, temporary files)."""


def _png_bytes(buf):
    """Minimal PNG writer (8-bit RGB / RGBA), no external imaging library needed."""
    h, w, ch = buf.shape
    ctype = {3: 2, 4: 6}[ch]
    raw = np.empty((h, 1 + w * ch), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = buf.reshape(h, w * ch)
    def chunk(tag, data):
        body = tag + data
        return struct.pack('>I', len(data)) + body + struct.pack('>I', zlib.crc32(body) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, ctype, 0, 0, 0))
            + chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) + chunk(b'IEND', b''))


def _tiff_bytes(buf):
    """Baseline little-endian TIFF, uncompressed, one strip; 8- or 16-bit, 1/3/4 samples per pixel."""
    buf = np.ascontiguousarray(buf)
    if buf.ndim == 2:
        buf = buf[:, :, None]
    h, w, ch = buf.shape
    bits = buf.dtype.itemsize * 8
    data = buf.astype('<u%d' % buf.dtype.itemsize).tobytes()
    entries = []        # (tag, type, count, value or bytes)
    extra = b''
    def add(tag, typ, values):
        nonlocal extra
        fmt = {3: 'H', 4: 'I'}[typ]
        raw = struct.pack('<%d%s' % (len(values), fmt), *values)
        if len(raw) <= 4:
            entries.append((tag, typ, len(values), raw.ljust(4, b'\0')))
        else:
            entries.append((tag, typ, len(values), None))
            extra += raw
            entries[-1] = (tag, typ, len(values), ('off', len(extra) - len(raw)))
    n_ifd = 10 + (1 if ch in (2, 4) else 0)
    ifd_off = 8
    extra_off = ifd_off + 2 + 12 * n_ifd + 4
    add(256, 4, [w]); add(257, 4, [h]); add(258, 3, [bits] * ch); add(259, 3, [1])
    add(262, 3, [2 if ch >= 3 else 1])
    add(273, 4, [0])                    # strip offset, patched below
    add(277, 3, [ch]); add(278, 4, [h]); add(279, 4, [len(data)]); add(284, 3, [1])
    if ch in (2, 4):
        add(338, 3, [2])                # ExtraSamples: unassociated alpha
    assert len(entries) == n_ifd
    data_off = extra_off + len(extra)
    out = [b'II*\0' + struct.pack('<I', ifd_off), struct.pack('<H', n_ifd)]
    for tag, typ, count, val in sorted(entries):
        if tag == 273:
            val = struct.pack('<I', data_off)
        elif isinstance(val, tuple):
            val = struct.pack('<I', extra_off + val[1])
        out.append(struct.pack('<HHI', tag, typ, count) + val)
    out.append(struct.pack('<I', 0))
    return b''.join(out) + extra + data


class PILOutput(Output):
    """8-bit stills: jpeg (Pillow) and png (Pillow, or the built-in writer without it);
    same file naming as cuburn/output.py:69-108."""

    def __init__(self, codec='jpeg', quality=100, alpha=False):
        self.type, self.quality, self.alpha = codec, quality, alpha
        if codec == 'jpeg':
            import PIL.Image      # noqa: F401  (fail at construction, like the reference)
        self.suffix = get_suffix(codec, alpha)

    def _save(self, arr):
        out = io.BytesIO()
        arr = np.ascontiguousarray(arr)
        try:
            import PIL.Image
            PIL.Image.fromarray(arr).save(out, self.type, quality=self.quality)
        except ImportError:
            if self.type != 'png':
                raise
            out.write(_png_bytes(arr if arr.ndim == 3 else np.repeat(arr[:, :, None], 3, 2)))
        out.seek(0)
        return out

    def encode(self, buf):
        if buf is None:
            return {}, []
        if self.type == 'jpeg':
            if self.alpha:
                return {'_color.jpg': self._save(buf[:, :, :3]), '_alpha.jpg': self._save(buf[:, :, 3])}, []
            return {'.jpg': self._save(buf[:, :, :3])}, []
        return {'.' + self.type: self._save(buf)}, []


class DeviceEncodedOutput(Output):
    """Stills encoded on the device: the frame leaves the GPU as a finished file.  The host frame is a byte buffer: a 16-byte
    record (u32 nbytes, status, a parameter of the encoder, 0 — an APNG frame block's number of chunks), then the file.  A subclass names the library's entry point
    (``entry``), gives its one argument beyond the frame and the destination (``argument``; ``arguments`` where there are
    more) and the buffer's size (``capacity``), and says what the file is (``suffix``, ``noun``)."""

    def shape(self, dim):
        return (self.capacity(dim),)

    def arguments(self):
        return (self.argument(),)

    def copy(self, fb, dim, pool=None, stream=None, dev_out=0, host=True):
        h_out = fb.host_buffer(self.shape(dim), self.dtype) if host else None
        _lib.check(getattr(_lib.load(), self.entry)(*((fb.ctx, dim.w, dim.h) + tuple(self.arguments())
                                                      + (h_out.ctypes.data if host else None, int(dev_out), self.capacity(dim)))))
        return h_out

    @staticmethod
    def file_bytes(buf, noun):
        """The file behind the record of a host frame, as a view of ``buf``; raises when the record says it did not fit."""
        nbytes, status = (int(v) for v in np.frombuffer(buf[:8], '<u4'))
        if status:
            raise _lib.FlameError('the %s needs %d bytes and the frame buffer holds %d' % (noun, nbytes, buf.size - 16))
        return buf[16:16 + nbytes]

    def encode(self, buf):
        if buf is None:
            return {}, []
        return {self.suffix: io.BytesIO(self.file_bytes(buf, self.noun).tobytes())}, []


class DeviceJPEGOutput(DeviceEncodedOutput):
    """JPEG stills encoded on the device (``output: {"type": "jpeg", "device": true, "quality": 1..100, "sampling": "444" |
    "420", "optimize": bool}``): a baseline file, 4:4:4 unless ``sampling`` says 4:2:0 (include/flame_hip.h, fl_output_jpeg and
    fl_output_jpeg_s).  ``optimize``: Huffman tables built from each frame's own symbol counts, as libjpeg's and Pillow's
    ``optimize`` (fl_output_jpeg_f with FL_JPEG_OPTIMIZE): the same coefficients in a smaller file, for some more time on the GPU.
    The record's parameter is the restart interval."""
    suffix, entry, noun = '.jpg', 'fl_output_jpeg', 'JPEG stream'

    def __init__(self, quality=100, alpha=False, sampling='444', optimize=False):
        if alpha:
            raise ValueError('the device JPEG encoder has no alpha plane: use "device": false with "alpha"')
        self.quality, self.alpha = _int_in('quality', quality, 1, 100), False
        self.sampling = _one_of('sampling', str(sampling), _lib.JPEG_SAMPLING, '"444" or "420"')
        self.optimize = _bool('optimize', optimize)
        if optimize:
            self.entry = 'fl_output_jpeg_f'
        elif self.sampling != '444':            # (4:4:4 stays on the entry point it has always used)
            self.entry = 'fl_output_jpeg_s'

    def argument(self):
        return self.quality

    def arguments(self):
        if self.optimize:
            return (self.quality, _lib.JPEG_SAMPLING[self.sampling], _lib.JPEG_OPTIMIZE)
        return (self.quality,) if self.sampling == '444' else (self.quality, _lib.JPEG_SAMPLING[self.sampling])

    @staticmethod
    def capacity(dim):
        """Record, header and twice the raw planes: a stream that needs more (noise at quality 100 takes 0.65 of raw) is
        reported by ``encode`` with the size it needs."""
        return 16 + _lib.JPEG_HEADER_BYTES + 2 * 3 * dim.w * dim.h


class DevicePNGOutput(DeviceEncodedOutput):
    """PNG stills encoded on the device (``output: {"type": "png", "encoder": "device", "alpha": bool, "bits": 8 | 16,
    "filter": "paeth" | "adaptive"}``): a truecolour file, filtered and deflated in independent segments (include/flame_hip.h,
    fl_output_png and fl_output_png_f).  ``bits``: 16 writes the samples of the 16-bit outputs (tiff, raw16) losslessly.
    ``filter``: every row Paeth, or each row the type of least cost (libpng's minimum sum of absolute differences).  The
    record's parameter is the segment's bytes."""
    suffix, entry, noun = '.png', 'fl_output_png', 'PNG file'

    def __init__(self, alpha=False, bits=8, filter='paeth'):
        self.alpha, self.bits = _bool('alpha', alpha), _bits(bits)
        self.filter = _one_of('filter', filter, _lib.PNG_FILTERS, '"paeth" or "adaptive"')
        self.channels = 4 if alpha else 3
        self.extended = bits != 8 or filter != 'paeth'          # (the defaults stay on the entry points they have always used)
        if self.extended:
            self.entry = 'fl_output_png_f'

    def argument(self):
        return self.channels

    def arguments(self):
        if self.extended:
            return (self.channels, self.bits, _lib.PNG_FILTERS[self.filter])
        return (self.channels,)

    def capacity(self, dim):
        """The library's bound: no frame needs more (noise is stored, at 17 bytes per segment above its own size)."""
        if self.extended:
            return int(_lib.load().fl_png_bound_f(dim.w, dim.h, self.channels, self.bits, _lib.PNG_FILTERS[self.filter]))
        return int(_lib.load().fl_png_bound(dim.w, dim.h, self.channels))


class PNGOutput(PILOutput):
    def __init__(self, alpha=False):
        PILOutput.__init__(self, 'png', alpha=alpha)

    def encode(self, buf):
        if buf is None:
            return {}, []
        img = buf if self.alpha else buf[:, :, :3]
        return {'.png': io.BytesIO(_png_bytes(np.ascontiguousarray(img)))}, []


class TiffOutput(Output):
    """16-bit stills (cuburn/output.py:110-136), written by the built-in baseline TIFF writer."""
    fmt = 1
    dtype = 'u2'
    suffix = '.tiff'

    def __init__(self, alpha=False):
        self.alpha = alpha

    def encode(self, buf):
        if buf is None:
            return {}, []
        return {'.tiff': io.BytesIO(_tiff_bytes(buf if self.alpha else buf[:, :, :3]))}, []


class DeviceTIFFOutput(DeviceEncodedOutput):
    """TIFF stills encoded on the device (``output: {"type": "tiff", "compression": "deflate", "alpha": bool}``): the samples of
    ``TiffOutput`` in a tiled file, Adobe deflate with the horizontal predictor (include/flame_hip.h, fl_output_tiff).  A profile
    gives 16 bits; ``bits=8`` writes the samples of the 8-bit outputs.  The record's parameter is a tile's bytes."""
    suffix, entry, noun = '.tiff', 'fl_output_tiff', 'TIFF file'

    def __init__(self, alpha=False, bits=16):
        self.alpha, self.bits = _bool('alpha', alpha), _bits(bits, 'bits')
        self.channels = 4 if alpha else 3

    def arguments(self):
        return (self.channels, self.bits)

    def capacity(self, dim):
        """The library's bound: no frame needs more (noise is stored, at 12 bytes per tile above its own size)."""
        return int(_lib.load().fl_tiff_bound(dim.w, dim.h, self.channels, self.bits))


class DeviceEXROutput(DeviceEncodedOutput):
    """OpenEXR stills encoded on the device (``output: {"type": "exr", "pixel": "half" | "float", "alpha": bool}``): the float
    picture as the filter chain left it, with no dither and no clamp, in a tiled ZIP file (include/flame_hip.h, fl_output_exr).
    There is no host writer behind it.  The record's parameter is a full tile's bytes."""
    suffix, entry, noun = '.exr', 'fl_output_exr', 'OpenEXR file'

    def __init__(self, alpha=False, pixel='half'):
        self.alpha, self.pixel = _bool('alpha', alpha), _one_of('pixel', pixel, _lib.EXR_PIXELS, '"half" or "float"')
        self.channels = 4 if alpha else 3

    def arguments(self):
        return (self.channels, _lib.EXR_PIXELS[self.pixel])

    def capacity(self, dim):
        """The library's bound: no frame needs more (a file of noise is exactly that long)."""
        return int(_lib.load().fl_exr_bound(dim.w, dim.h, self.channels, _lib.EXR_PIXELS[self.pixel]))


class RawOutput(Output):
    suffix = '.rgba8'


class Raw16Output(Output):
    fmt = 1
    dtype = 'u2'
    suffix = '.rgba16'


_VIDEO = ('x264', 'vp8', 'vp9', 'prores', 'mjpeg', 'gif', 'webp', 'apng')


def get_suffix(codec, alpha=False):
    ext = dict(jpeg='.jpg', png='.png', tiff='.tiff', exr='.exr', raw='.rgba8', raw16='.rgba16', x264='.h264',
               prores='.mov', vp8='.webm', vp9='.webm', mjpeg='.avi', gif='.gif', webp='.webp', apng='.apng')[codec]
    if codec in ('webp', 'apng'):                        # alpha travels inside the one file
        return ext
    return ('_color' + ext) if alpha else ext


# The outputs the device alone writes: their class (where it lives in encoders.py, by name: that module imports this one), the
# keys their ``output`` block may hold in the order the refusal names them, and what the refusal calls them.
_DEVICE_OUTPUTS = {
    'exr': (DeviceEXROutput, ('pixel', 'alpha'), 'the device OpenEXR encoder'),
    'gif': ('GIFOutput', ('colors', 'dither', 'loop'), 'the device GIF encoder'),
    'webp': ('WebPOutput', ('alpha', 'loop'), 'the device WebP encoder'),
    'apng': ('APNGOutput', ('alpha', 'bits', 'filter', 'loop'), 'the device APNG encoder'),
    'png': (DevicePNGOutput, ('alpha', 'bits', 'filter'), 'the device PNG encoder'),
    'tiff': (DeviceTIFFOutput, ('alpha',), 'output.compression: the device TIFF encoder'),
}


def _device_output(kind, opts, **more):
    """The device's output of this kind from the keys left in ``opts``; no key of another encoder means anything to it."""
    cls, keys, who = _DEVICE_OUTPUTS[kind]
    extra = sorted(set(opts) - set(keys))
    if extra:
        quoted = ['"%s"' % k for k in keys]
        takes = quoted[0] if len(keys) == 1 else ', '.join(quoted[:-1]) + ' and ' + quoted[-1]
        raise ValueError('%s takes %s only, not %s' % (who, takes, ', '.join(extra)))
    if isinstance(cls, str):
        from . import encoders
        cls = getattr(encoders, cls)
    return cls(**dict(opts, **more))


def get_output_for_profile(gprof):
    """Output module for the profile's ``output`` block (cuburn/output.py:421-436)."""
    opts = dict(gprof.output.raw())
    handler = opts.pop('type', 'jpeg')
    if handler == 'exr':
        return _device_output('exr', opts)
    if 'pixel' in opts:
        raise ValueError('output.pixel: only exr takes it, not "%s"' % handler)
    if handler in ('gif', 'webp', 'apng'):               # formats of their own, on the device only
        return _device_output(handler, opts, fps=gprof.fps)
    for key in ('colors', 'dither', 'loop'):
        if key in opts:
            raise ValueError('output.%s: only gif%s, not "%s"' % (key, ', webp and apng take it' if key == 'loop' else ' takes it', handler))
    if not (handler == 'png' and opts.get('encoder') == 'device'):
        for key in ('bits', 'filter'):
            if key in opts:
                raise ValueError('output.%s: only the device PNG encoder takes it: set "encoder": "device" on a png output' % key)
    compression = opts.pop('compression', None)
    if compression is not None:
        if handler != 'tiff':
            raise ValueError('output.compression: only tiff takes it, not "%s"' % handler)
        _one_of('compression', compression, ('none', 'deflate'), '"none" or "deflate"')
    if opts.pop('device', False):
        if handler != 'jpeg':
            raise ValueError('output.device: only jpeg is encoded on the device, not "%s"' % handler)
        return DeviceJPEGOutput(**opts)
    encoder = opts.pop('encoder', None)
    if encoder is not None:
        if encoder != 'device':
            raise ValueError('output.encoder: "device" is the only encoder to choose, not "%s"' % (encoder,))
        if handler != 'png':
            raise ValueError('output.encoder: selects the device PNG encoder ("device": true is the JPEG switch), not "%s"' % handler)
        return _device_output('png', opts)
    if 'optimize' in opts and handler != 'mjpeg':
        raise ValueError('output.optimize: only the device JPEG encoder optimises its Huffman tables: '
                         'set "device": true on a jpeg output, or use mjpeg')
    if handler in ('jpeg', 'png'):
        return PILOutput(codec=handler, **opts)
    if handler == 'tiff':
        if compression == 'deflate':                     # the device's file; "none", or no key: the host writer, as before
            return _device_output('tiff', opts)
        return TiffOutput(**opts)
    if handler == 'raw':
        return RawOutput()
    if handler == 'raw16':
        return Raw16Output()
    if handler in _VIDEO:
        from . import encoders
        if handler == 'x264':
            return encoders.X264Output(**opts)
        if handler == 'prores':
            return encoders.ProResOutput(fps=gprof.fps, **opts)
        if handler == 'mjpeg':
            return encoders.MJPEGOutput(fps=gprof.fps, **opts)
        return encoders.VPxOutput(codec=handler, fps=gprof.fps, **opts)
    raise ValueError('Invalid output type "%s".' % handler)


def get_suffix_for_profile(gprof):
    opts = dict(gprof.output.raw())
    return get_suffix(opts.get('type', 'jpeg'), bool(opts.get('alpha')))




class Proxy(object):
    """One entry of the profile's ``proxies``: a smaller copy of every frame.  ``gprof`` is the profile as this copy sees it (its
    own width, height and output block), ``out`` its output module, ``suffix`` what its files carry in front of the extension."""

    def __init__(self, width, height, suffix, gprof, out):
        self.width, self.height, self.suffix, self.gprof, self.out = width, height, suffix, gprof, out


def _subsamples_chroma(out):
    """The output halves the chroma planes, so the frame's sides must be even."""
    return (getattr(out, 'sampling', None) == '420' or getattr(out, 'fmt', None) == _lib.OUT['yuv420p10']
            or getattr(out, 'csp', None) == 'i420' or (hasattr(out, 'csp') and bool(getattr(out, 'alpha', False)))      # (x264's alpha stream is i420)
            or (getattr(out, 'pix_fmt', '') or '').startswith('yuv420'))


def proxy_entries(gprof):
    """The profile's ``proxies`` as ``[(width, height, suffix, output block)]``, from the largest to the smallest, every rule of
    the key checked (sizes, ratio, suffixes) except what needs the output module."""
    raw = gprof.raw().get('proxies') or []
    if not isinstance(raw, (list, tuple)):
        raise ValueError('proxies must be a list of {"width", "height", "suffix", "output"} entries')
    W, H = int(gprof.width), int(gprof.height)
    master = dict(gprof.output.raw())
    entries, seen = [], {}
    for k, ent in enumerate(raw):
        who = 'proxies[%d]' % k
        if not isinstance(ent, dict):
            raise ValueError('%s must be an object with "width" and "height"' % who)
        unknown = sorted(set(ent) - set(('width', 'height', 'suffix', 'output')))
        if unknown:
            raise ValueError('%s: unknown key %s' % (who, ', '.join(unknown)))
        size = []
        for key in ('width', 'height'):
            v = ent.get(key)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError('%s.%s must be a positive integer' % (who, key))
            size.append(v)
        w, h = size
        if w > W or h > H:
            raise ValueError('%s: %d x %d is larger than the master\'s %d x %d (enlarging is not supported)' % (who, w, h, W, H))
        suffix = ent.get('suffix', '_%dp' % h)
        if not isinstance(suffix, str) or not suffix:
            raise ValueError('%s.suffix must be a non-empty string: without one its files would replace the master\'s' % who)
        if suffix in seen:
            raise ValueError('%s and proxies[%d] have the same suffix "%s"' % (who, seen[suffix], suffix))
        seen[suffix] = k
        block = ent.get('output', master)
        if not isinstance(block, dict):
            raise ValueError('%s.output must be an output block' % who)
        entries.append((w, h, suffix, dict(block), k))
    entries.sort(key=lambda e: (-e[0] * e[1], e[4]))            # each is made from the one before it, the largest from the master
    w0, h0, src = W, H, 'the master'
    for w1, h1, _, _, k1 in entries:
        if w1 > w0 or h1 > h0:
            raise ValueError('proxies[%d] (%d x %d) is made from %s (%d x %d), the next larger frame, and is larger than it '
                             'on an axis' % (k1, w1, h1, src, w0, h0))
        if w0 > RESIZE_MAX_RATIO * w1 or h0 > RESIZE_MAX_RATIO * h1:
            raise ValueError('proxies[%d]: %d x %d is less than 1/%d of %s (%d x %d), the frame it is made from, on an axis; '
                             'list a size in between' % (k1, w1, h1, RESIZE_MAX_RATIO, src, w0, h0))
        w0, h0, src = w1, h1, 'proxies[%d]' % k1
    return entries


def get_proxies_for_profile(gprof):
    """``[Proxy]`` for the profile's ``proxies`` key, from the largest to the smallest, each with a fresh output module from
    get_output_for_profile.  A profile without the key gives ``[]``."""
    out = []
    for w, h, suffix, block, k in proxy_entries(gprof):
        doc = dict(gprof.raw(), width=w, height=h, output=block)
        doc.pop('proxies', None)
        view = gprof.rebuilt(doc)
        try:
            mod = get_output_for_profile(view)
        except ValueError as e:
            raise ValueError('proxies[%d].%s' % (k, e))
        if _subsamples_chroma(mod) and (w % 2 or h % 2):
            raise ValueError('proxies[%d]: %d x %d has an odd side, and its output subsamples the chroma 4:2:0' % (k, w, h))
        out.append(Proxy(w, h, suffix, view, mod))
    return out


def get_proxy_files_for_profile(gprof):
    """``[suffix + extension]`` of the files the profile's proxies add to every output, without building an output module."""
    return [suffix + get_suffix(block.get('type', 'jpeg'), bool(block.get('alpha'))) for _, _, suffix, block, _ in proxy_entries(gprof)]
