"""The portable form of one stream of a batch (Batch.save_streams / load_streams; include/glv_spectrum.h), restated in numpy: where the regions of a blob
lie, how to view them, and the rotation (`unrotate`) that takes a ring as the batch keeps it to the order a blob holds it in.  Host code only -- the library's kernel
(glava_amd/csrc/glv_slots.hip) does the moving; this is the layout the tests index blobs with and a host may read a downloaded blob by.

A blob is, in this order and present regions only (desc.regions):

    bit 0  gravity rows   [2][n] elements        the stream's two rows of the gravity store
    bit 1  average ring   [2][F][n] elements     oldest frame first: row q is ring slot (head + q) mod F; row F - 1 is the newest
    bit 2  s16 PCM ring   [n][2] int16           oldest frame first: frame q is ring frame (ring position + q) mod n
    bit 3  f32 PCM ring   [n][2] float32         likewise

elements are float32 (desc.elem_bytes 4) or GL_R16 texels, uint16 (2).

DensePool is the other half of a service's bookkeeping: which slots of a batch hold listeners, kept as a prefix (Batch.process_first_* / copy_streams)."""
from __future__ import annotations

import numpy as np

REGION_GRAVITY, REGION_AVERAGE, REGION_RING_S16, REGION_RING_F32 = 1, 2, 4, 8
REGION_NAMES = {REGION_GRAVITY: "gravity", REGION_AVERAGE: "average", REGION_RING_S16: "ring_s16", REGION_RING_F32: "ring_f32"}


def _field(desc, name):
    return int(desc[name] if isinstance(desc, dict) else getattr(desc, name))


def region_shapes(desc) -> dict:
    """{name: (dtype, shape)} of the regions a blob of `desc` holds, in blob order"""
    n, F, elem, regions = (_field(desc, k) for k in ("n", "avg_frames", "elem_bytes", "regions"))
    if elem not in (2, 4):
        raise ValueError(f"elem_bytes={elem}: 4 (float state) or 2 (GL_R16 texels)")
    if regions & ~15:
        raise ValueError(f"regions=0x{regions:x}: bits 0..3")
    state = np.dtype(np.float32 if elem == 4 else np.uint16)
    out = {}
    if regions & REGION_GRAVITY:
        out["gravity"] = (state, (2, n))
    if regions & REGION_AVERAGE:
        out["average"] = (state, (2, F, n))
    if regions & REGION_RING_S16:
        out["ring_s16"] = (np.dtype(np.int16), (n, 2))
    if regions & REGION_RING_F32:
        out["ring_f32"] = (np.dtype(np.float32), (n, 2))
    return out


def region_offsets(desc) -> dict:
    """{name: (first byte, bytes)} of the regions within one stream's blob, in blob order"""
    out, at = {}, 0
    for name, (dt, shape) in region_shapes(desc).items():
        nbytes = int(np.prod(shape)) * dt.itemsize
        out[name] = (at, nbytes)
        at += nbytes
    return out


def stream_bytes(desc) -> int:
    """bytes of one stream's blob: what the library reports as desc.bytes"""
    return sum(nbytes for _, nbytes in region_offsets(desc).values())


def split_blob(desc, blob) -> dict:
    """views of one stream's blob (uint8 [stream_bytes], a numpy array) by region: {name: array of the region's dtype and shape}"""
    blob = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    if blob.size != stream_bytes(desc):
        raise ValueError(f"blob of {blob.size} bytes, the descriptor says {stream_bytes(desc)}")
    shapes, out = region_shapes(desc), {}
    for name, (at, nbytes) in region_offsets(desc).items():
        dt, shape = shapes[name]
        out[name] = blob[at:at + nbytes].view(dt).reshape(shape)
    return out


def unrotate(rows, pos: int, axis: int = 0):
    """a ring as the batch keeps it -> the order a blob holds it in: entry q of the result is entry (pos + q) mod len of `rows` along `axis` (pos = head for
    the average ring's slots, the ring position for a PCM ring's frames: the oldest entry first)"""
    rows = np.asarray(rows)
    m = rows.shape[axis]
    if not 0 <= pos < m:
        raise ValueError(f"pos={pos}: must be in [0, {m})")
    return np.roll(rows, -pos, axis=axis)


class DensePool:
    """The listeners of one batch kept dense in slots [0, active), so that every update is Batch.process_first_*(active, ...): host bookkeeping only, the
    caller issues the device calls it names.

        slot = pool.attach()            # then batch.reset_streams([slot])
        move = pool.detach(slot)        # (src, dst): then batch.copy_streams([dst], batch, [src]); None: the slot was the last one
        pool.grow(new_capacity)         # then new_batch.copy_streams(range(active), old_batch, range(active)): the slots keep their numbers

    A listener that detach moved is now known by `dst`: the caller renames it."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError(f"capacity={capacity}: must be >= 1")
        self.capacity, self.active = int(capacity), 0

    def attach(self) -> int:
        if self.active == self.capacity:
            raise IndexError(f"all {self.capacity} slots are taken: grow() first")
        self.active += 1
        return self.active - 1

    def detach(self, slot: int):
        if not 0 <= slot < self.active:
            raise IndexError(f"slot={slot}: the active slots are [0, {self.active})")
        self.active -= 1
        return None if slot == self.active else (self.active, slot)

    def grow(self, new_capacity: int) -> None:
        if new_capacity < self.capacity:
            raise ValueError(f"new_capacity={new_capacity}: below the capacity {self.capacity}")
        self.capacity = int(new_capacity)
