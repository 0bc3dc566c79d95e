"""numpy restatement of one image-pool query (include/gan_amd.h, gan_pool_exchange): the counter hash, fill / swap / keep,
images taken in batch order.  Values are only moved: the GPU kernel is compared with this bit for bit."""
import numpy as np

M64 = (1 << 64) - 1
STREAM_Y, STREAM_X = 32, 33


def mix64(z):
    """gan_amd/csrc/elementwise.hip: mix64 (the splitmix64 finaliser), on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def decisions(batch, capacity, seed, stream_id, stored, launches):
    """-> ([(kind, slot)] per image in batch order, new stored); kind 'fill' | 'swap' | 'keep', slot None for keep."""
    key = mix64((seed & M64) ^ ((launches & 0xffffffff) << 32) ^ stream_id)
    out = []
    for b in range(batch):
        h = mix64(key ^ b)
        if stored < capacity:
            out.append(('fill', stored))
            stored += 1
        elif h >> 63:
            out.append(('swap', ((h & 0xffffffff) * capacity) >> 32))
        else:
            out.append(('keep', None))
    return out, stored


def query(images, pool, state, seed, stream_id):
    """images [B, ...], pool [P, ...] (same trailing shape and dtype), state (stored, launches)
    -> (out [B, ...], new pool, new state, trace); the arguments are left unchanged."""
    images = np.asarray(images)
    pool = np.array(pool, copy=True)
    stored, launches = int(state[0]), int(state[1])
    trace, _ = decisions(images.shape[0], pool.shape[0], seed, stream_id, stored, launches)
    out = np.empty_like(images)
    for b, (kind, j) in enumerate(trace):
        if kind == 'fill':
            pool[j] = images[b]
            out[b] = images[b]
        elif kind == 'swap':
            out[b] = pool[j]          # (a copy: the slot is overwritten next)
            pool[j] = images[b]
        else:
            out[b] = images[b]
    return out, pool, (min(pool.shape[0], stored + images.shape[0]), launches + 1), trace


def run_trace(capacity, batch, seed, stream_id, launches):
    """The decision traces of `launches` successive queries of an empty pool."""
    stored, traces = 0, []
    for n in range(launches):
        t, stored = decisions(batch, capacity, seed, stream_id, stored, n)
        traces.append(t)
    return traces


def same_slot_swaps(trace):
    """Does one launch swap the same slot twice or more?"""
    slots = [j for kind, j in trace if kind == 'swap']
    return len(slots) != len(set(slots))


# the parameter sets of the GPU kernel tests: (capacity, batch)
GPU_CASES = [(3, 2), (1, 4), (4, 16)]
GPU_SEED = 123
GPU_LAUNCHES = 6
