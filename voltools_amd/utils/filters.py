"""Filter taps for ``StaticVolume.filter_stack``."""
import numpy as np

AVAILABLE_WINDOWS = ('ramp', 'shepp-logan', 'cosine', 'hamming', 'hann')


def ramp_taps(extent: int, window: str = 'ramp', half_width=None) -> np.ndarray:
    """The taps of the ramp filter of weighted back-projection for lines of ``extent`` samples at unit spacing: float64, symmetric about
    the middle tap, ``(2 extent - 1,)`` -- every tap a line of that length can reach -- or ``(2 half_width + 1,)``, the middle of that row
    (``0 <= half_width <= extent - 1``).  With ``m`` the offset from the middle tap:

    * ``'ramp'``: the band-limited ramp (Ram-Lak) in closed form, ``t[0] = 1/4``, ``t[m] = -1 / (pi m)**2`` for odd ``m`` and exactly 0
      for even ``m``: ``filter_stack`` skips zero taps, so half of the row costs nothing;
    * ``'shepp-logan'``: ``-2 / (pi**2 (4 m**2 - 1))``;
    * ``'cosine'``, ``'hamming'``, ``'hann'``: the Ram-Lak taps zero-padded to a power of two ``>= 2 extent``, their real DFT multiplied
      by ``cos(pi f)``, ``0.54 + 0.46 cos(2 pi f)`` or ``0.5 + 0.5 cos(2 pi f)`` over the frequency ``f`` in cycles per sample
      (``|f| <= 1/2``), and inverted (Kak & Slaney's recipe, in numpy float64)."""
    if isinstance(extent, bool) or not isinstance(extent, (int, np.integer)) or extent < 1:
        raise ValueError('extent must be a positive int')
    if window not in AVAILABLE_WINDOWS:
        raise ValueError(f'window must be one of {AVAILABLE_WINDOWS}')
    extent = int(extent)
    if half_width is None:
        half_width = extent - 1
    if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or not 0 <= half_width <= extent - 1:
        raise ValueError(f'half_width must be an int inside [0, {extent - 1}]')
    r = extent - 1
    m = np.arange(-r, r + 1)
    if window == 'shepp-logan':
        t = -2.0 / (np.pi ** 2 * (4.0 * m.astype(np.float64) ** 2 - 1.0))
    else:
        t = np.zeros(2 * r + 1, dtype=np.float64)
        odd = (m % 2) != 0
        t[odd] = -1.0 / (np.pi * m[odd].astype(np.float64)) ** 2
        t[r] = 0.25
        if window != 'ramp':
            size = 1 << int(np.ceil(np.log2(2 * extent)))
            ring = np.zeros(size, dtype=np.float64)
            ring[m % size] = t                                # offset m at index m mod size: a real, even sequence
            f = np.fft.rfftfreq(size)
            win = {'cosine': np.cos(np.pi * f), 'hamming': 0.54 + 0.46 * np.cos(2 * np.pi * f), 'hann': 0.5 + 0.5 * np.cos(2 * np.pi * f)}[window]
            ring = np.fft.irfft(np.fft.rfft(ring).real * win, size)
            t = ring[m % size]
            t = 0.5 * (t + t[::-1])                           # symmetric to the last bit
    return np.ascontiguousarray(t[r - half_width:r + half_width + 1])
