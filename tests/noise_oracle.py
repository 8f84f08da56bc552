"""Pure-Python restatement of the device noise source (ragraph_amd/csrc/rng.h): splitmix64 on (seed, row, draw) with 64-bit
masking and the high-half reduction to [0, N).  tests/test_cpu_noise_device.py pins it; tests/test_gpu_noise_device.py holds
ragraph_noise_rows_i64 to it bit for bit."""
M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def lp_draw(seed: int, row: int, draw: int) -> int:
    return splitmix64((splitmix64((seed ^ splitmix64(row & M64)) & M64) + draw) & M64)


def lp_below(h: int, m: int) -> int:
    return (h * m) >> 64


def noise_row(seed: int, row: int, j: int, n: int) -> int:
    return lp_below(lp_draw(seed & M64, row, j), n)


def noise_rows(seed: int, row_ids, m: int, n: int):
    """[[noise_row(seed, r, j, n) for j < m] for r in row_ids]."""
    return [[noise_row(seed, int(r), j, n) for j in range(m)] for r in row_ids]
