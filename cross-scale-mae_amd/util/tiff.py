"""Baseline TIFF reader in pure Python / numpy for multi-band tiles (EuroSAT's 13-band Sentinel-2 GeoTIFFs): the reference opens them with
rasterio (util/datasets.py:545-549), which is not a dependency here.

`read_tiff(path) -> numpy [H, W, C]` (uint8 or uint16) reads the first image of a classic TIFF, little- or big-endian, stored in strips, with
`BitsPerSample` 8 or 16 unsigned, `SamplesPerPixel` 1..16, chunky or planar `PlanarConfiguration`, `Compression` 1 (none) or 8 / 32946 (deflate,
through zlib) with `Predictor` 1.  Anything else — BigTIFF, tiles, LZW, predictor 2, float or signed samples, ... — raises ValueError naming
the tag and its value.  Tags the reader does not know (the GeoTIFF keys among them) are ignored."""
import struct
import zlib

import numpy as np

# tag -> name, for the tags that are read
IMAGE_WIDTH, IMAGE_LENGTH, BITS_PER_SAMPLE, COMPRESSION, PHOTOMETRIC, STRIP_OFFSETS, SAMPLES_PER_PIXEL, ROWS_PER_STRIP = 256, 257, 258, 259, 262, 273, 277, 278
STRIP_BYTE_COUNTS, PLANAR_CONFIGURATION, PREDICTOR, TILE_WIDTH, TILE_OFFSETS, SAMPLE_FORMAT = 279, 284, 317, 322, 324, 339
_TYPE = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d"}   # TIFF field type -> struct code
_WANTED = {IMAGE_WIDTH, IMAGE_LENGTH, BITS_PER_SAMPLE, COMPRESSION, STRIP_OFFSETS, SAMPLES_PER_PIXEL, ROWS_PER_STRIP, STRIP_BYTE_COUNTS,
           PLANAR_CONFIGURATION, PREDICTOR, TILE_WIDTH, TILE_OFFSETS, SAMPLE_FORMAT}


def _ifd(buf, order, path):
    """The wanted tags of the first image file directory as tag -> tuple of ints."""
    (offset,) = struct.unpack_from(order + "I", buf, 4)
    if offset + 2 > len(buf):
        raise ValueError(f"{path}: the first directory lies outside the file")
    (count,) = struct.unpack_from(order + "H", buf, offset)
    tags = {}
    for k in range(count):
        at = offset + 2 + 12 * k
        if at + 12 > len(buf):
            raise ValueError(f"{path}: the first directory is cut short")
        tag, ftype, n = struct.unpack_from(order + "HHI", buf, at)
        if tag not in _WANTED:
            continue
        code = _TYPE.get(ftype)
        if code is None or code in ("c", "f", "d", "II", "ii"):
            raise ValueError(f"{path}: tag {tag} has field type {ftype}, not an integer type")
        size = struct.calcsize(code) * n
        pos = at + 8 if size <= 4 else struct.unpack_from(order + "I", buf, at + 8)[0]
        if pos + size > len(buf):
            raise ValueError(f"{path}: the values of tag {tag} lie outside the file")
        tags[tag] = struct.unpack_from(f"{order}{n}{code}", buf, pos)
    return tags


def read_tiff(path):
    """-> numpy [H, W, C] uint8 / uint16 (native byte order) of the first image in `path`; see the module docstring for what is read."""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 8 or buf[:2] not in (b"II", b"MM"):
        raise ValueError(f"{path}: not a TIFF file (byte-order mark {buf[:2]!r})")
    order = "<" if buf[:2] == b"II" else ">"
    (magic,) = struct.unpack_from(order + "H", buf, 2)
    if magic != 42:
        raise ValueError(f"{path}: TIFF version {magic} is not read (42 = classic TIFF; 43 = BigTIFF)")
    tags = _ifd(buf, order, path)

    def one(tag, default=None):
        if tag not in tags:
            if default is None:
                raise ValueError(f"{path}: tag {tag} is missing")
            return default
        return int(tags[tag][0])

    if TILE_WIDTH in tags or TILE_OFFSETS in tags:
        raise ValueError(f"{path}: TileWidth (tag {TILE_WIDTH}) = {tags.get(TILE_WIDTH, ('set',))[0]}: tiled layout is not read, only strips")
    W, H, C = one(IMAGE_WIDTH), one(IMAGE_LENGTH), one(SAMPLES_PER_PIXEL, 1)
    if not 1 <= C <= 16:
        raise ValueError(f"{path}: SamplesPerPixel (tag {SAMPLES_PER_PIXEL}) = {C}: 1..16 are read")
    if W < 1 or H < 1:
        raise ValueError(f"{path}: ImageWidth / ImageLength (tags {IMAGE_WIDTH} / {IMAGE_LENGTH}) = {W} / {H}")
    bits = tags.get(BITS_PER_SAMPLE, (1,))
    if len(set(bits)) != 1 or bits[0] not in (8, 16) or len(bits) not in (1, C):
        raise ValueError(f"{path}: BitsPerSample (tag {BITS_PER_SAMPLE}) = {bits}: 8 or 16 bits, the same for every sample, are read")
    fmt = tags.get(SAMPLE_FORMAT, (1,))
    if any(v != 1 for v in fmt):
        raise ValueError(f"{path}: SampleFormat (tag {SAMPLE_FORMAT}) = {fmt}: only unsigned integers (1) are read")
    compression = one(COMPRESSION, 1)
    if compression not in (1, 8, 32946):
        raise ValueError(f"{path}: Compression (tag {COMPRESSION}) = {compression}: 1 (none) and 8 / 32946 (deflate) are read")
    predictor = one(PREDICTOR, 1)
    if predictor != 1:
        raise ValueError(f"{path}: Predictor (tag {PREDICTOR}) = {predictor}: only 1 (none) is read")
    planar = one(PLANAR_CONFIGURATION, 1)
    if planar not in (1, 2):
        raise ValueError(f"{path}: PlanarConfiguration (tag {PLANAR_CONFIGURATION}) = {planar}")
    rows = min(one(ROWS_PER_STRIP, H), H)
    if rows < 1:
        raise ValueError(f"{path}: RowsPerStrip (tag {ROWS_PER_STRIP}) = {rows}")
    offsets, counts = tags.get(STRIP_OFFSETS), tags.get(STRIP_BYTE_COUNTS)
    if offsets is None:
        raise ValueError(f"{path}: tag {STRIP_OFFSETS} (StripOffsets) is missing")
    per_plane = -(-H // rows)
    planes, chans = (C, 1) if planar == 2 else (1, C)    # planes in the file, samples per pixel within one
    if len(offsets) != planes * per_plane or (counts is not None and len(counts) != len(offsets)):
        raise ValueError(f"{path}: StripOffsets (tag {STRIP_OFFSETS}) holds {len(offsets)} strips, {planes * per_plane} expected")
    dtype = np.dtype("u1" if bits[0] == 8 else order + "u2")
    out = np.empty((planes, H, W, chans), dtype=dtype.newbyteorder("="))
    for p in range(planes):
        for s in range(per_plane):
            k = p * per_plane + s
            r0 = s * rows
            nrows = min(rows, H - r0)
            need = nrows * W * chans * dtype.itemsize
            if compression == 1:
                data = buf[offsets[k]:offsets[k] + need]
            else:
                if counts is None:
                    raise ValueError(f"{path}: tag {STRIP_BYTE_COUNTS} (StripByteCounts) is missing in a compressed file")
                if offsets[k] + counts[k] > len(buf):
                    raise ValueError(f"{path}: strip {k} lies outside the file")
                data = zlib.decompress(buf[offsets[k]:offsets[k] + counts[k]])[:need]
            if len(data) < need:
                raise ValueError(f"{path}: strip {k} holds {len(data)} bytes, {need} expected")
            out[p, r0:r0 + nrows] = np.frombuffer(data, dtype=dtype, count=nrows * W * chans).reshape(nrows, W, chans)
    return np.ascontiguousarray(out[0] if planar == 1 else out[..., 0].transpose(1, 2, 0))
