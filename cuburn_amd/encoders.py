"""
Video outputs: the device converts a frame to the pixel format an external encoder takes, the host
feeds the encoder's stdin and hands back the finished segment when the stream is flushed.

Role of cuburn/output.py:139-409 (ProResOutput, X264Output, VPxOutput): same constructor options,
same encoder command lines, same ``encode(buf) -> (media, logs)`` protocol (``encode(None)``
flushes; a change of frame size flushes the x264 stream and starts a new one).  The encoders are
separate programs (x264, vpxenc, ffmpeg) found on PATH at the first frame — ``command=`` replaces
the program name, which is also how the tests drive the classes without them.

MJPEGOutput needs no program: the device encodes every frame as a JPEG (output.DeviceJPEGOutput) and the host
only puts the frames into an AVI file.  GIFOutput needs none either: the device writes every frame's block, palette and
LZW data included, and the host puts the blocks into a GIF89a file.  WebPOutput likewise: the device writes every frame as a
lossless `VP8L` chunk and the host puts the chunks into a RIFF file, a still's or an animation's.
APNGOutput likewise: the device writes every frame's `IDAT` or `fdAT` chunks, numbered and checksummed, and the host puts
`fcTL`s between them and the header chunks in front.
"""
import collections
import fractions
import struct
import subprocess
import tempfile
import zlib

import numpy as np

from . import _lib
from .output import DeviceEncodedOutput, DeviceJPEGOutput, Output, _bits, _bool, _int_in, _one_of


class _EncoderPipe(object):
    """One running encoder: frames go to its stdin; its stdout (or a named file it writes itself)
    is the media segment, its stderr the log."""

    def __init__(self, argv, what, named_suffix=None):
        self.what = what
        self.named = tempfile.NamedTemporaryFile(suffix=named_suffix) if named_suffix else None
        self.outf = None if named_suffix else tempfile.TemporaryFile()
        argv = [str(a) for a in argv] + ([self.named.name] if self.named else [])
        self.errf = tempfile.TemporaryFile()        # a file, not a pipe: a chatty encoder can never block on it
        try:
            self.proc = subprocess.Popen(argv, stdin=subprocess.PIPE, stdout=self.outf if self.outf else subprocess.DEVNULL,
                                         stderr=self.errf)
        except OSError as e:
            raise IOError('cannot start %s (%s): %s' % (what, argv[0], e))

    def _log(self):
        self.errf.seek(0)
        return self.errf.read().decode('utf-8', 'replace')

    def write(self, buf):
        try:
            self.proc.stdin.write(memoryview(np.ascontiguousarray(buf)).cast('B'))
        except (IOError, OSError) as e:
            raise IOError('%s stopped reading frames: %s\n%s' % (self.what, e, self._log()))

    def abort(self):
        """Kill the encoder and drop its temporary files (a failed job must leave nothing running)."""
        for step in (lambda: self.proc.stdin.close(), self.proc.kill, self.proc.wait, self.errf.close,
                     lambda: self.outf and self.outf.close(), lambda: self.named and self.named.close()):
            try:
                step()
            except Exception:
                pass

    def finish(self):
        """Close stdin, wait for the encoder; returns (media file positioned at 0, log text)."""
        try:
            self.proc.stdin.close()
        except (IOError, OSError):
            pass
        self.proc.wait()
        log = self._log()
        self.errf.close()
        if self.proc.returncode:
            raise IOError('%s exited with an error\n%s' % (self.what, log))
        if self.named:
            media = open(self.named.name, 'rb')     # keep a handle, let the name go (output.py:176-179)
            self.named.close()
        else:
            media = self.outf
            media.seek(0)
        return media, log


def _abort_pipes(obj, names):
    for n in names:
        pipe = getattr(obj, n, None)
        if pipe is not None:
            pipe.abort()
            setattr(obj, n, None)


class _PlanarOutput(Output):
    """Outputs whose device format is planar: ``copy`` shapes per cuburn/output.py:323-338."""
    pix_fmt = 'yuv444p'

    def abort(self):
        _abort_pipes(self, ('_pipe',))

    def shape(self, dim):
        if self.fmt == _lib.OUT['yuv420p10']:
            return (dim.h * dim.w * 6 // 4,)
        return (3, dim.h, dim.w)


class ProResOutput(_PlanarOutput):
    """12-bit 4:4:4 studio-swing frames into ``ffmpeg -c:v prores`` (cuburn/output.py:139-187)."""
    fmt = _lib.OUT['yuv444p12']
    dtype = 'u2'

    def __init__(self, fps=24, command='ffmpeg'):
        self.fps, self.command = fps, command
        self._pipe = None
        self._dim = None

    def convert(self, fb, gprof, dim, stream=None):
        self._dim = (dim.w, dim.h)

    def copy(self, fb, dim, *args, **kwargs):
        self._dim = (dim.w, dim.h)
        return super(ProResOutput, self).copy(fb, dim, *args, **kwargs)

    def encode(self, buf):
        if buf is None:
            if self._pipe is None:
                return {}, []
            media, _ = self._pipe.finish()
            self._pipe = None
            return {'.mov': media}, []
        if self._pipe is None:
            w, h = self._dim if self._dim else (buf.shape[2], buf.shape[1])
            argv = [self.command] + ('-loglevel panic -f rawvideo -pix_fmt yuv444p12le -s %dx%d -r %s -i - '
                                     '-c:v prores -f mov -y' % (w, h, self.fps)).split()
            self._pipe = _EncoderPipe(argv, 'ffmpeg', named_suffix='.mov')
        self._pipe.write(buf)
        return {}, []


class X264Output(Output):
    """16-bit RGB frames into x264 (high 4:4:4 by default); with ``alpha`` a second encoder receives
    the alpha plane as the luma of a 4:2:0 stream with neutral chroma (cuburn/output.py:190-293)."""
    fmt = _lib.OUT['rgba16']
    dtype = 'u2'

    profiles = {'normal': '--profile high444 --level 4.2', '': ''}
    base = '--no-progress --input-depth 16 --sync-lookahead 0 --rc-lookahead 5 --muxer raw -o - - --log-level debug'

    def __init__(self, profile='normal', csp='i444', crf=15, command='x264', x264opts='', alpha=False):
        self.args = ' '.join([command, self.base, self.profiles[profile], '--crf', str(crf), x264opts]).split()
        self.alpha, self.csp = alpha, csp
        self.framesize = None
        self._color = self._alpha = None
        self._neutral = None

    def _start(self, framesize, alpha):
        extras = ['--input-csp', 'yv12' if alpha else 'rgb', '--demuxer', 'raw', '--input-res', '%dx%d' % (framesize[1], framesize[0])]
        extras += ['--output-csp', 'i420', '--chroma-qp-offset', '24'] if alpha else ['--output-csp', self.csp]
        return _EncoderPipe(self.args + extras, 'x264')

    def abort(self):
        _abort_pipes(self, ('_color', '_alpha'))

    def _flush(self):
        if self._color is None:
            return {}, []
        media, log = self._color.finish()
        self._color = None
        if not self.alpha:
            return {'.h264': media}, [('x264_color', log)]
        amedia, alog = self._alpha.finish()
        self._alpha = None
        return {'_color.h264': media, '_alpha.h264': amedia}, [('x264_color', log), ('x264_alpha', alog)]

    def encode(self, buf):
        out = ({}, [])
        if buf is None or self.framesize != tuple(buf.shape[:2]):
            out = self._flush()
        if buf is None:
            return out
        if self._color is None:
            self.framesize = tuple(buf.shape[:2])
            self._color = self._start(self.framesize, False)
            if self.alpha:
                try:
                    self._alpha = self._start(self.framesize, True)
                except IOError:                     # do not leave the colour encoder running without its twin
                    self._color.abort(); self._color = None
                    raise
                self._neutral = np.full(self.framesize[0] * self.framesize[1] // 2, 32767, dtype='u2')   # both chroma planes
        try:
            self._color.write(buf[:, :, :3])
            if self.alpha:
                self._alpha.write(buf[:, :, 3])
                self._alpha.write(self._neutral)
        except IOError:
            self.abort()                            # neither encoder survives a failed write
            raise
        return out


class VPxOutput(_PlanarOutput):
    """Planar YUV frames into vpxenc (cuburn/output.py:295-409).  ``pix_fmt``: yuv420p (8-bit 4:4:4
    from the device, chroma decimated on the host as the reference does), and for vp9 yuv444p,
    yuv420p10, yuv444p10, yuv444p12."""

    base = 'vpxenc --end-usage=3 -p 1 -q --cpu-used=-8 --lag-in-frames=5 --min-q=2 --disable-kf --arnr-maxframes=3 -o - -'
    _formats = {                  # pix_fmt: (device format, dtype, extra arguments)
        'yuv420p': ('yuv444p', 'u1', []),
        'yuv444p': ('yuv444p', 'u1', ['--profile=1', '--i444']),
        'yuv420p10': ('yuv420p10', 'u2', ['-b', '10', '--input-bit-depth=10', '--profile=2']),
        'yuv444p10': ('yuv444p10', 'u2', ['-b', '10', '--input-bit-depth=10', '--profile=3', '--i444']),
        'yuv444p12': ('yuv444p12', 'u2', ['-b', '12', '--input-bit-depth=12', '--profile=3', '--i444']),
    }

    def __init__(self, codec='vp9', fps=24, crf=15, pix_fmt='yuv420p', command=None):
        if pix_fmt not in self._formats:
            raise ValueError('Invalid pix_fmt: ' + pix_fmt)
        if pix_fmt != 'yuv420p' and codec != 'vp9':
            raise ValueError('%s needs codec vp9' % pix_fmt)
        self.codec, self.pix_fmt = codec, pix_fmt
        dev, self.dtype, extra = self._formats[pix_fmt]
        self.fmt = _lib.OUT[dev]
        self.args = self.base.split() + extra + ['--codec=' + codec, '--cq-level=' + str(crf), '--fps=%d/1' % fps]
        if command:
            self.args[0] = command
        if codec == 'vp9':
            self.args += ['-t', '4']
        self._pipe = None
        self._dim = None

    def convert(self, fb, gprof, dim, stream=None):
        self._dim = (dim.w, dim.h)

    def copy(self, fb, dim, *args, **kwargs):
        self._dim = (dim.w, dim.h)
        return super(VPxOutput, self).copy(fb, dim, *args, **kwargs)

    def encode(self, buf):
        if buf is None:
            if self._pipe is None:
                return {}, []
            media, log = self._pipe.finish()
            self._pipe = None
            return {'.webm': media}, [('webm', log)]
        if self._pipe is None:
            w, h = self._dim if self._dim else (buf.shape[2], buf.shape[1])
            extras = ['-w', w, '-h', h]
            columns = int(max(0, min(3, np.log2(w) - 8.9)))
            if columns:
                extras.append('--tile-columns=%d' % columns)
            self._pipe = _EncoderPipe(self.args + extras, 'vpxenc')
        if self.pix_fmt == 'yuv420p':
            self._pipe.write(buf[0])
            self._pipe.write(buf[1, ::2, ::2])
            self._pipe.write(buf[2, ::2, ::2])
        else:
            self._pipe.write(buf)
        return {}, []


AVI_MAX_BYTES = 2 ** 31 - 1       # AVI 1.0: sizes and offsets are u32 and players read them as signed; OpenDML is not written
_AVI_MOVI_DATA = 224              # RIFF 12, LIST hdrl 8 + 192, LIST movi 12: where the first chunk's header lies
_JPEG_SOF0 = 158                  # offset of the SOF0 segment in the device's header: SOI 2, APP0 18, DQT 2 x 69


def _avi_header(w, h, fps, sizes, movi_bytes):
    """Everything in front of the first chunk (AVI 1.0, little-endian).  sizes: the unpadded chunk sizes; movi_bytes: the
    chunks with their headers and padding."""
    n, largest = len(sizes), max(sizes) if sizes else 0
    rate = fractions.Fraction(fps).limit_denominator(100000)
    avih = struct.pack('<14I', int(round(1e6 / fps)), 0, 0, 0x10, n, 0, 1, largest, w, h, 0, 0, 0, 0)      # 0x10: AVIF_HASINDEX
    strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, largest,
                       0xffffffff, 0, 0, 0, w, h)
    strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', w * h * 3, 0, 0, 0, 0)
    assert len(avih) == 56 and len(strh) == 56 and len(strf) == 40

    def chunk(tag, body):
        return tag + struct.pack('<I', len(body)) + body

    def lst(tag, body):
        return b'LIST' + struct.pack('<I', 4 + len(body)) + tag + body
    hdrl = lst(b'hdrl', chunk(b'avih', avih) + lst(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf)))
    riff = 4 + len(hdrl) + 12 + movi_bytes + 8 + 16 * n
    out = b'RIFF' + struct.pack('<I', riff) + b'AVI ' + hdrl + b'LIST' + struct.pack('<I', 4 + movi_bytes) + b'movi'
    assert len(out) == _AVI_MOVI_DATA
    return out


def frame_ticks(k, fps, per_second):
    """How many ticks (``per_second`` of them a second) frame k lasts: round(u (k + 1) / fps) - round(u k / fps) with
    u = per_second, so a file keeps the rate on average."""
    return int(round(float(per_second) * (k + 1) / fps)) - int(round(float(per_second) * k / fps))


class _FrameFile(object):
    """What the animations the device writes frame by frame share (mixed into a DeviceEncodedOutput): the temporary file, its frame
    count and frame size, ``abort``, and ``encode(buf)`` — ``None`` flushes; else the block behind the record is parsed for its
    size, a size other than the last flushes and starts a new file (as X264Output does), the first frame of a file writes the
    header, and the frame's wrapper and the block, copied out of the pinned buffer, follow.  A subclass supplies ``_parse(data)
    -> (h, w)`` or raises, ``_header() -> bytes``, ``_wrap(data) -> (bytes in front, bytes behind)``, which may refuse the
    frame, and ``_finish() -> the complete file``."""

    @staticmethod
    def _need_fps(name, fps, most=None, why=None):
        if not fps > 0:
            raise ValueError('%s needs fps above 0' % name)
        if most is not None and fps > most:
            raise ValueError('%s: fps %g gives frames of %s: use %d or less' % (name, fps, why, most))

    def _reset(self):
        self._file, self._nframes, self.framesize = None, 0, None

    def abort(self):
        if self._file is not None:
            self._file.close()
        self._reset()

    def _flush(self):
        if self._nframes == 0:
            return {}, []
        f = self._finish()
        f.seek(0)
        self._reset()
        return {self.suffix: f}, []

    def _add(self, data):
        front, behind = self._wrap(data)
        if self._file is None:
            self._file = tempfile.TemporaryFile()
            self._file.write(self._header())
        self._file.write(front)
        self._file.write(memoryview(np.ascontiguousarray(data)))      # the pinned frame buffer is reused by the next frame: the bytes are copied out here
        self._file.write(behind)
        self._nframes += 1

    def encode(self, buf):
        if buf is None:
            return self._flush()
        data = self.file_bytes(buf, self.noun)
        size, out = self._parse(data), ({}, [])
        if self.framesize != size:
            out = self._flush()
            self.framesize = size
        self._add(data)
        return out


class MJPEGOutput(_FrameFile, DeviceJPEGOutput):
    """Animations as Motion-JPEG in an AVI 1.0 file (``output: {"type": "mjpeg", "quality": 1..100, "sampling": "420" | "444",
    "optimize": bool}``, ``--codec mjpeg``; ``optimize`` as DeviceJPEGOutput's, every frame with tables of its own): every frame leaves the GPU as a finished baseline JPEG (``copy`` is DeviceJPEGOutput's) and becomes a
    ``00dc`` chunk; ``encode(None)`` writes the header and the ``idx1`` index and returns the file.  No external program.
    A change of frame size flushes and starts a new file, as X264Output does."""
    suffix = '.avi'

    def __init__(self, fps=24, quality=90, sampling='420', alpha=False, optimize=False):
        if alpha:
            raise ValueError('mjpeg has no alpha plane: use x264 with "alpha"')
        self._need_fps('mjpeg', fps)
        DeviceJPEGOutput.__init__(self, quality=quality, sampling=sampling, optimize=optimize)
        self.fps = fps
        self._reset()

    def _reset(self):
        _FrameFile._reset(self)
        self._sizes, self._movi = [], 0

    def _parse(self, data):
        if len(data) < _JPEG_SOF0 + 9 or bytes(data[_JPEG_SOF0:_JPEG_SOF0 + 2]) != b'\xff\xc0':
            raise IOError('the frame is not a JPEG stream of the device encoder')
        return struct.unpack('>HH', bytes(data[_JPEG_SOF0 + 5:_JPEG_SOF0 + 9]))      # (height, width)

    def _header(self):
        return b'\0' * _AVI_MOVI_DATA                  # its place: written at the flush, when the sizes are known

    def _wrap(self, data):
        n = len(data)
        if _AVI_MOVI_DATA + self._movi + 8 + n + (n & 1) + 8 + 16 * (len(self._sizes) + 1) > AVI_MAX_BYTES:
            raise IOError('the AVI file would pass %d bytes at frame %d: render shorter files with "shard" (--shard SECS)'
                          % (AVI_MAX_BYTES, len(self._sizes) + 1))
        self._sizes.append(n)
        self._movi += 8 + n + (n & 1)
        return b'00dc' + struct.pack('<I', n), b'\0' * (n & 1)

    def _finish(self):
        f, off = self._file, 4
        index = bytearray()
        for n in self._sizes:                     # offsets count from the 'movi' fourcc
            index += struct.pack('<4sIII', b'00dc', 0x10, off, n)       # 0x10: AVIIF_KEYFRAME
            off += 8 + n + (n & 1)
        f.write(b'idx1' + struct.pack('<I', len(index)) + index)
        f.seek(0)
        f.write(_avi_header(self.framesize[1], self.framesize[0], self.fps, self._sizes, self._movi))
        return f


def gif_delays(nframes, fps):
    """Centiseconds of frames 0 .. nframes - 1 (frame_ticks at 100 a second)."""
    return [frame_ticks(k, fps, 100) for k in range(nframes)]


class GIFOutput(_FrameFile, DeviceEncodedOutput):
    """Animations as a looping GIF89a file (``output: {"type": "gif", "colors": 2..256, "dither": "ordered" | "none",
    "loop": 0..65535}``, ``--codec gif``): every frame leaves the GPU as a finished frame block with a palette of its own — median
    cut, ordered dither, LZW (include/flame_hip.h, fl_output_gif) — and the host writes the header, the NETSCAPE2.0 loop
    extension (``loop`` 0: forever), a graphic control extension with the frame's delay in front of every block, and the trailer.
    ``encode(None)`` returns the file.  No external program.  A change of frame size flushes and starts a new file, as X264Output
    does.  The record's parameter is the LZW segment's pixels."""
    suffix, entry, noun = '.gif', 'fl_output_gif', 'GIF frame block'

    def __init__(self, fps=24, colors=256, dither='ordered', loop=0):
        self._need_fps('gif', fps, 50, 'less than 2 centiseconds, which browsers play at 10')
        self.fps, self.colors = fps, _int_in('colors', colors, 2, 256)
        self.dither = _one_of('dither', dither, _lib.GIF_DITHER, '"ordered" or "none"')
        self.loop = _int_in('loop', loop, 0, 65535)
        self._reset()

    def arguments(self):
        return (self.colors, _lib.GIF_DITHER[self.dither])

    def capacity(self, dim):
        """The library's bound: no frame needs more (twelve bits a pixel and the segments' framing)."""
        return int(_lib.load().fl_gif_bound(dim.w, dim.h))

    def _parse(self, data):
        if len(data) < _lib.GIF_HEADER_BYTES + 2 or data[0] != 0x2c or data[9] != 0x87:
            raise IOError('the frame is not a block of the device GIF encoder')
        w, h = struct.unpack('<HH', bytes(data[5:9]))
        return h, w

    def _header(self):
        h, w = self.framesize
        return (b'GIF89a' + struct.pack('<HH', w, h) + b'\x70\x00\x00'      # no global table, 8 bits a primary
                + b'\x21\xff\x0bNETSCAPE2.0\x03\x01' + struct.pack('<H', self.loop) + b'\x00')

    def _wrap(self, data):
        delay = frame_ticks(self._nframes, self.fps, 100)
        return b'\x21\xf9\x04\x04' + struct.pack('<H', delay) + b'\x00\x00', b''      # disposal 1: leave the frame in place

    def _finish(self):
        self._file.write(b'\x3b')
        return self._file


def webp_duration(k, fps):
    """Milliseconds of frame k (frame_ticks at 1000 a second)."""
    return frame_ticks(k, fps, 1000)


def webp_durations(nframes, fps):
    return [webp_duration(k, fps) for k in range(nframes)]


def _u24(v):
    return struct.pack('<I', v)[:3]


class WebPOutput(_FrameFile, DeviceEncodedOutput):
    """Stills and animations as lossless WebP (``output: {"type": "webp", "alpha": bool, "loop": 0..65535}``, ``--codec webp``):
    every frame leaves the GPU as a finished `VP8L` chunk — subtract green, a predictor mode per 16 x 16 tile, prefix codes per
    64 x 64 tile (include/flame_hip.h, fl_output_webp) — and the host writes the RIFF file around the chunks.  A file that ends
    with one frame is the simple format (`RIFF`, size, `WEBP`, the chunk), so the first chunk is held back until a second frame or
    the flush decides; a file of two or more is the extended format: `VP8X`, `ANIM` (background 0, ``loop``, 0: forever), one
    `ANMF` per frame with its duration in milliseconds, not blended, not disposed.  ``encode(None)`` returns the file.  No
    external program.  A change of frame size flushes and starts a new file, as GIFOutput does.  The record's parameter is
    PB | EB << 8, the tiles' size bits."""
    suffix, entry, noun = '.webp', 'fl_output_webp', 'WebP frame block'
    LIMIT = (1 << 32) - 10                 # a RIFF size is 32 bits
    _HEAD = 12 + 18 + 14                   # `RIFF`, `VP8X` and `ANIM` in front of an animation's frames
    _TOO_LONG = 'the WebP file would pass 4 GiB: use shard to split the animation into several files'

    def __init__(self, fps=24, alpha=False, loop=0):
        self._need_fps('webp', fps, 90, '10 ms or less, which players show for 100 ms')
        self.fps, self.alpha, self.loop = fps, _bool('alpha', alpha), _int_in('loop', loop, 0, 65535)
        self.channels = 4 if alpha else 3
        self._reset()

    def _reset(self):
        _FrameFile._reset(self)
        self._first, self._size = None, 0      # the frame held back (it counts as one while it is); the bytes of the animation's `ANMF`s

    def argument(self):
        return self.channels

    def capacity(self, dim):
        """The library's bound: no frame needs more (60 bits a pixel and the codes' headers)."""
        return int(_lib.load().fl_webp_bound(dim.w, dim.h, self.channels))

    def _parse(self, data):
        if len(data) < 8 + 5 or bytes(data[:4]) != b'VP8L' or data[8] != 0x2f or len(data) & 1:
            raise IOError('the frame is not a block of the device WebP encoder')
        bits, = struct.unpack('<I', bytes(data[9:13]))
        return (bits >> 14 & 0x3fff) + 1, (bits & 0x3fff) + 1

    def _header(self):
        h, w = self.framesize
        return (b'RIFF\0\0\0\0WEBP' + b'VP8X' + struct.pack('<I', 10) + bytes([0x12 if self.alpha else 0x02, 0, 0, 0]) + _u24(w - 1) + _u24(h - 1)
                + b'ANIM' + struct.pack('<IIH', 6, 0, self.loop))

    def _wrap(self, block):
        h, w = self.framesize
        dur = webp_duration(self._nframes, self.fps)
        if self._HEAD + self._size + 24 + len(block) > self.LIMIT:
            self.abort()
            raise IOError(self._TOO_LONG)
        self._size += 24 + len(block)
        return b'ANMF' + struct.pack('<I', 16 + len(block)) + _u24(0) + _u24(0) + _u24(w - 1) + _u24(h - 1) + _u24(dur) + b'\x02', b''

    def _add(self, data):
        if self._nframes == 0:                              # the first frame of a file: held back, copied out of the pinned buffer
            block = bytes(memoryview(np.ascontiguousarray(data)))
            if 12 + len(block) > self.LIMIT:
                raise IOError(self._TOO_LONG)
            self._first, self._nframes = block, 1
            return
        if self._first is not None:                         # a second frame: the file is an animation
            first, self._first, self._nframes = self._first, None, 0
            _FrameFile._add(self, first)
        _FrameFile._add(self, data)

    def _finish(self):
        if self._first is not None:                         # one frame: the simple format
            f = tempfile.TemporaryFile()
            f.write(b'RIFF' + struct.pack('<I', 4 + len(self._first)) + b'WEBP')
            f.write(self._first)
            return f
        self._file.seek(4)
        self._file.write(struct.pack('<I', self._HEAD + self._size - 8))
        return self._file


def apng_delay(fps):
    """(delay_num, delay_den) of every frame: 1 / fps as an exact fraction of seconds (24 -> 1/24, 30000/1001 -> 1001/30000).
    Raises where the fraction does not fit the fcTL's two u16."""
    f = fractions.Fraction(fps).limit_denominator(1001) if fps > 0 else fractions.Fraction(0)
    if not 0 < f.numerator <= 65535:
        raise ValueError('apng: fps %g gives a frame delay of %d/%d s, which does not fit 16 bits' % (fps, f.denominator, f.numerator))
    return f.denominator, f.numerator


def _png_chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


class APNGOutput(_FrameFile, DeviceEncodedOutput):
    """Animations as APNG (``output: {"type": "apng", "bits": 8 | 16, "alpha": bool, "filter": "paeth" | "adaptive", "loop":
    0..65535}``, ``--codec apng``): lossless, 8 or 16 bits a sample, and a PNG reader that knows no animation shows frame 0.
    Every frame leaves the GPU as its finished chunks — the device PNG's zlib stream as `IDAT`s for frame 0 and as `fdAT`s, sequence
    numbers and CRCs included, for every later one (include/flame_hip.h, fl_output_apng) — and the host writes the signature,
    `IHDR`, `acTL` (``loop`` plays, 0: forever), an `fcTL` in front of every block (the whole frame, delay 1 / fps as an exact
    fraction, no disposal, no blending) and `IEND`.  ``encode(None)`` patches the frame count into `acTL` and returns the file.
    No external program.  A change of frame size flushes and starts a new file, as GIFOutput does.

    Sequence numbers: with n chunks a frame (``fl_apng_chunks``), frame 0's `fcTL` is 0 and frame k >= 1 holds
    1 + (k - 1)(n + 1) in its `fcTL` and the n numbers behind it in its `fdAT`s.  A frame is numbered when it is queued
    (``number``, which ``copy`` calls), one frame ahead of ``encode``; ``encode`` takes a block only where it starts with the tag
    and number the file needs next.  The record's parameter is the segment's bytes, its fourth word the number of chunks."""
    suffix, entry, noun = '.apng', 'fl_output_apng', 'APNG frame block'
    _ACTL = 8 + 25                          # where `acTL` lies: behind the signature and IHDR

    def __init__(self, fps=24, alpha=False, bits=8, filter='paeth', loop=0):
        self._need_fps('apng', fps, 90, '10 ms or less, which players show for 100 ms')      # (webp's cap, taken over as a stated condition: DESIGN §4.17)
        self.delay = apng_delay(fps)
        self.fps, self.alpha, self.bits = fps, _bool('alpha', alpha), _bits(bits)
        self.filter = _one_of('filter', filter, _lib.PNG_FILTERS, '"paeth" or "adaptive"')
        self.loop, self.channels = _int_in('loop', loop, 0, 65535), 4 if alpha else 3
        self._reset()
        self._queued = collections.deque()      # (w, h, chunks a frame, first number) of the frames numbered and not yet encoded
        self._qsize, self._qframes = None, 0    # the size and count of the frames numbered for the file being queued

    def chunks(self, w, h):
        return int(_lib.load().fl_apng_chunks(w, h, self.channels, self.bits))

    @staticmethod
    def first_number(k, n):
        """What frame k's block starts with: FL_APNG_IDAT for the `IDAT`s of frame 0, else its first `fdAT`'s number."""
        return _lib.APNG_IDAT if k == 0 else 2 + (k - 1) * (n + 1)

    def number(self, w, h):
        """Number the next frame to be queued (w x h; another size than the last starts a new file): returns the ``seq`` of
        fl_output_apng.  ``encode`` expects the frames' blocks in the order of these calls."""
        if self._qsize != (h, w):
            self._qsize, self._qframes = (h, w), 0
        n = self.chunks(w, h)
        if n == 0:
            raise ValueError('apng: no frame of %d x %d' % (w, h))
        seq = self.first_number(self._qframes, n)
        if seq != _lib.APNG_IDAT and seq + n - 1 > 0xfffffffe:
            raise IOError('the APNG file would run out of sequence numbers at frame %d: render shorter files with "shard" (--shard SECS)'
                          % self._qframes)
        self._queued.append((w, h, n, seq))
        self._qframes += 1
        return seq

    def arguments(self):
        return (self.channels, self.bits, _lib.PNG_FILTERS[self.filter])

    def capacity(self, dim):
        """The library's bound: no frame needs more (the device PNG's, and 4 bytes a chunk)."""
        return int(_lib.load().fl_apng_bound(dim.w, dim.h, self.channels, self.bits, _lib.PNG_FILTERS[self.filter]))

    def copy(self, fb, dim, pool=None, stream=None, dev_out=0, host=True):
        h_out = fb.host_buffer(self.shape(dim), self.dtype) if host else None
        seq = self.number(dim.w, dim.h)
        try:
            _lib.check(_lib.load().fl_output_apng(*((fb.ctx, dim.w, dim.h) + self.arguments()
                                                    + (seq, h_out.ctypes.data if host else None, int(dev_out), self.capacity(dim)))))
        except Exception:
            self._queued.pop()                  # nothing was queued: the number is free again
            self._qframes -= 1
            raise
        return h_out

    def abort(self):
        _FrameFile.abort(self)
        self._queued.clear()
        self._qsize, self._qframes = None, 0

    def encode(self, buf):
        if buf is None:
            if self._queued:                    # frames numbered for this file that never arrived
                self.abort()
                raise IOError('the APNG file was flushed with numbered frames still to come')
            self._qsize, self._qframes = None, 0
            return self._flush()
        if not self._queued:
            raise IOError('an APNG frame block that was never numbered: number(w, h) comes before encode')
        w, h, n, _ = self._queued.popleft()
        try:
            self._frame = (w, h, n, int(np.frombuffer(buf[12:16], '<u4')[0]))      # what _parse and _wrap go by: the last is the record's chunks
            return _FrameFile.encode(self, buf)
        except Exception:
            self.abort()                        # a frame is missing: no file with a gap, what was written goes
            raise

    def _parse(self, data):
        w, h = self._frame[:2]                  # (the block does not say: the frame was numbered with its size)
        return h, w

    def _header(self):
        h, w = self.framesize
        return (b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, self.bits, 6 if self.alpha else 2, 0, 0, 0))
                + _png_chunk(b'acTL', struct.pack('>II', 0, self.loop)))      # the frame count: patched at the flush

    def _wrap(self, data):
        w, h, n, nchunks = self._frame
        want = self.first_number(self._nframes, n)
        tag = b'IDAT' if want == _lib.APNG_IDAT else b'fdAT'
        head = bytes(data[4:8]) if want == _lib.APNG_IDAT else bytes(data[4:12])
        if nchunks != n or len(data) < 12 or head != (tag if want == _lib.APNG_IDAT else tag + struct.pack('>I', want)):
            raise IOError('frame %d of the APNG file needs a block of %d chunks that starts with %s%s; the block has %d and starts with %r'
                          % (self._nframes, n, tag.decode(), '' if want == _lib.APNG_IDAT else ' %d' % want, nchunks, head))
        fctl = 0 if self._nframes == 0 else want - 1
        return _png_chunk(b'fcTL', struct.pack('>IIIIIHHBB', fctl, w, h, 0, 0, self.delay[0], self.delay[1], 0, 0)), b''

    def _finish(self):
        f = self._file
        f.write(_png_chunk(b'IEND', b''))
        f.seek(self._ACTL)
        f.write(_png_chunk(b'acTL', struct.pack('>II', self._nframes, self.loop)))
        return f
