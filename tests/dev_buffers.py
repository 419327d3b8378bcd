"""Device buffers for the GPU tests: arrays uploaded with sentinel bytes around them, and the two helpers every file used to carry.  A plain module: the `gpu`
fixture and the stop-after-a-device-error fixture stay with the test files."""
import numpy as np

SENTINEL = 0xA5
TAIL = 64    # sentinel bytes behind every DevBuffers buffer
GUARD = 32   # sentinel bytes on either side of every Dev buffer


def sentinel_like(img):
    return np.full(img.shape, SENTINEL, np.uint8)


def differing(got, want):
    """pixels (last axis = channels) that differ"""
    return int((got != want).any(axis=-1).sum())


class DevBuffers:
    """arrays uploaded to device allocations `lead` bytes in, with sentinel bytes before and behind; freed on exit"""
    def __init__(self, gpu, *arrays, lead=0):
        self.gpu, self.arrays, self.lead, self.bases = gpu, [np.ascontiguousarray(a, np.uint8) for a in arrays], lead, []

    def __enter__(self):
        ptrs = []
        for a in self.arrays:
            padded = np.concatenate([np.full(self.lead, SENTINEL, np.uint8), a.ravel(), np.full(TAIL, SENTINEL, np.uint8)])
            p = self.gpu.dev_alloc(padded.nbytes)
            self.bases.append(p)
            self.gpu.dev_upload(p, padded)
            ptrs.append(p + self.lead)
        return ptrs

    def surroundings_intact(self):
        for p, a in zip(self.bases, self.arrays):
            got = self.gpu.dev_download(p, (self.lead + a.size + TAIL,))
            if not ((got[:self.lead] == SENTINEL).all() and (got[self.lead + a.size:] == SENTINEL).all()):
                return False
        return True

    def __exit__(self, *exc):
        for p in self.bases:
            self.gpu.dev_free(p)


class Dev:
    """device copies of arrays between GUARD sentinel bytes, `offset` bytes past a 256-byte aligned address; freed on exit"""
    def __init__(self, gpu):
        self.gpu, self.blocks = gpu, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for base, _, _ in self.blocks.values():
            self.gpu.dev_free(base)

    def put(self, array, offset=0):
        a = np.ascontiguousarray(array)
        image = np.full(a.nbytes + 2 * GUARD, SENTINEL, np.uint8)
        image[GUARD + offset:GUARD + offset + a.nbytes] = a.reshape(-1).view(np.uint8)
        base = self.gpu.dev_alloc(image.nbytes)
        self.gpu.dev_upload(base, image)
        self.blocks[base + GUARD + offset] = (base, a.nbytes, offset)
        return base + GUARD + offset

    def sentinel(self, shape, offset=0):
        return self.put(np.full(shape, SENTINEL, np.uint8), offset)

    def get(self, ptr, shape):
        """the array, after checking that the guard bytes around it are intact"""
        base, nbytes, offset = self.blocks[ptr]
        image = self.gpu.dev_download(base, (nbytes + 2 * GUARD,))
        assert (image[:GUARD + offset] == SENTINEL).all() and (image[GUARD + offset + nbytes:] == SENTINEL).all(), "a write outside the buffer"
        return image[GUARD + offset:GUARD + offset + nbytes].reshape(shape)
