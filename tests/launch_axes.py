"""The launch grids of the likelihood grid (csrc/lnl.hip), the correlated grid (csrc/clnl.hip) and the per-realization
spectra (csrc/spectra.hip), restated in plain Python as functions of the sizes a caller chooses, and the GPU cases that
take every one of their launch axes past its first workgroup. tests/test_gpu_lnl.py, tests/test_gpu_clnl.py and
tests/test_gpu_spectra.py import the cases; tests/test_launch_axes_host.py holds the constants to the sources and the
cases to what they are there for, without a GPU. A change of a tile size fails there and asks for new shapes."""

# ----------------------------------------------------------------------------- the tiles, as the sources have them
LNL_GRID = 32        # lnl.hip kLnlGrid: grid points of a k_lnl_quad workgroup
LNL_RPAD = 32        # lnl.hip kLnlRpad: k_fit_apply's realization padding
LNL_GROUP = 16       # lnl_host.h groups_of: rows of U in a group, KG = ceil(K / 16)
LNL_KG_WIDE = 8      # lnl.hip lnl_launch: KG <= 8 runs k_lnl_quad<4>, above it k_lnl_quad<2>
LNL_NH = (4, 2)      # 16-realization blocks of a workgroup's tile, for KG <= LNL_KG_WIDE and above it
LNL_LDS = 65536      # bytes of LDS a workgroup may ask for
CLNL_RPAD = 32       # clnl.hip clnl_launch: k_fit_apply's realization padding
CLNL_TILE = 64       # clnl.hip / clnl_host.h pad64: realizations of a k_clnl_mix / k_clnl_solve workgroup
REAL_PAD = 128       # fpta_internal.h kRealPad: a synthesized block's realization padding
SPECTRA_AMP = 256    # spectra.hip k_spectra_amp: realizations of a workgroup
SPECTRA_SCALE = 512  # spectra.hip k_spectra_scale: realizations of a workgroup (256 threads, a pair each)


def _ceil(a, b):
    return -(-a // b)


def _fills(n, tile):
    """How many of each block's `tile` slots the n items fill, block by block."""
    return [min(tile, n - i) for i in range(0, n, tile)]


def lnl_launch(K, G, R):
    """k_lnl_quad's launch for K columns, G grid points and R realizations: the instance NH, the row groups KG, the
    dynamic LDS in bytes, R_pad, the grid extents n_rt (blockIdx.x) and n_gc (blockIdx.y), and per block of each axis
    the padded realizations, the realizations proper and the grid points it holds."""
    R_pad = _ceil(R, LNL_RPAD) * LNL_RPAD
    KG = _ceil(K, LNL_GROUP)
    nh = LNL_NH[0] if KG <= LNL_KG_WIDE else LNL_NH[1]
    tile = 16 * nh
    return dict(K=K, KG=KG, nh=nh, tile=tile, lds=8 * 16 * KG * tile, R_pad=R_pad, n_rt=_ceil(R_pad, tile),
                n_gc=_ceil(G, LNL_GRID), padded=_fills(R_pad, tile), real=_fills(R, tile), chunks=_fills(G, LNL_GRID))


def clnl_launch(R):
    """The realization axis of k_clnl_mix and k_clnl_solve: R_pad, vld, the tiles (blockIdx.x), and per tile the
    padded realizations (columns below R_pad; the rest of a tile is dead: V = 0, q not written) and the realizations
    proper."""
    R_pad = _ceil(R, CLNL_RPAD) * CLNL_RPAD
    vld = _ceil(R_pad, CLNL_TILE) * CLNL_TILE
    n = vld // CLNL_TILE
    pad = lambda m: _fills(m, CLNL_TILE) + [0] * (n - _ceil(m, CLNL_TILE))  # noqa: E731
    return dict(R_pad=R_pad, vld=vld, tiles=n, padded=pad(R_pad), real=pad(R))


def spectra_launch(R):
    """The realization axes of k_spectra_amp and k_spectra_scale: R_pad, the blocks of each (blockIdx.x) and the padded
    realizations each block holds."""
    R_pad = _ceil(R, REAL_PAD) * REAL_PAD
    return dict(R_pad=R_pad, amp=_ceil(R_pad, SPECTRA_AMP), scale=_ceil(R_pad, SPECTRA_SCALE),
                amp_fill=_fills(R_pad, SPECTRA_AMP), scale_fill=_fills(R_pad, SPECTRA_SCALE))


# ----------------------------------------------------------------------------- the GPU cases
# tests/test_gpu_lnl.py, stage 2: (P, N, G, R, empty) of quad_case, K = 2 N
LNL_STAGE2 = [
    (2, 2, 70, 130, True),     # K = 4 on <4>: realization tiles 64 + 64 + 32 of R_pad = 160; grid chunks 32 + 32 + 6
    (3, 9, 33, 65, False),     # two row groups; the second realization tile half full; a second chunk of one point
    (2, 64, 32, 128, False),   # K = 128, KG = 8: <4>'s full 64 KB of LDS; exactly two full tiles and one full chunk
    (2, 65, 33, 65, True),     # K = 130, the smallest <2> shape: three 32-wide tiles, two chunks
]
# the bitwise case: realizations and grid rows that sit at the edges of the tiles and chunks
LNL_BITWISE = dict(N=9, G=70, R=130, reals=(0, 63, 64, 128, 129), rows=(31, 32, 63, 64, 69))
# the batch path's second block: R realizations on an nA x ngamma grid (K = 10 there)
LNL_BATCH = dict(K=10, R=130, nA=9, ngamma=8)

# tests/test_gpu_clnl.py: R on the stage shapes (P, K, G), the bitwise picks, the batch path's second block
CLNL_R = 130
CLNL_STAGES = [(3, 4, 1), (5, 14, 3)]  # n = 12; n = 70: two block rows, Y_j is read back in tiles 1 and 2
CLNL_REALS = (0, 63, 64, 128, 129)

# tests/test_gpu_spectra.py: P pulsars of n TOAs with n_rn modes of red noise, R realizations from an odd real0
SPECTRA = dict(P=5, n=(40, 60), n_rn=3, R=520, real0=1001, picks=(0, 255, 256, 511, 512, 519), paths=(4, 3))
