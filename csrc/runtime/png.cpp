// PNG row un-filtering (utils/flow_io.py:read_png): the one sequential step of the decoder.
// A plain host function, called through ctypes on the loaded library (a ctypes call releases
// the GIL, so the loader's decode threads run it side by side); it is no torch op.
//
// rows: the inflated image data, H rows of 1 filter byte + rowbytes bytes, un-filtered in place
// (the filter bytes stay); bpp: bytes per complete pixel, at least 1.  Filter types 0..4 are
// None, Sub, Up, Average, Paeth; bytes left of the row and the row above the first are 0.
// Returns 0, -1 on bad arguments, or 1 + the row of the first filter byte above 4.
#include <cstdlib>

extern "C" int jr_png_unfilter(unsigned char* rows, int H, int rowbytes, int bpp) {
  if (!rows || H < 0 || rowbytes < 1 || bpp < 1) return -1;
  const long stride = (long)rowbytes + 1;
  for (int y = 0; y < H; ++y) {
    unsigned char* cur = rows + y * stride + 1;
    const unsigned char* up = y > 0 ? cur - stride : nullptr;
    const int n = rowbytes, head = bpp < n ? bpp : n;   // the first pixel has nothing to its left
    switch (cur[-1]) {
      case 0:
        break;
      case 1:
        for (int i = bpp; i < n; ++i) cur[i] = (unsigned char)(cur[i] + cur[i - bpp]);
        break;
      case 2:
        if (up)
          for (int i = 0; i < n; ++i) cur[i] = (unsigned char)(cur[i] + up[i]);
        break;
      case 3:
        for (int i = 0; i < head; ++i) cur[i] = (unsigned char)(cur[i] + ((up ? up[i] : 0) >> 1));
        for (int i = bpp; i < n; ++i) cur[i] = (unsigned char)(cur[i] + ((cur[i - bpp] + (up ? up[i] : 0)) >> 1));
        break;
      case 4:
        for (int i = 0; i < head; ++i) cur[i] = (unsigned char)(cur[i] + (up ? up[i] : 0));   // paeth(0, b, 0) = b
        for (int i = bpp; i < n; ++i) {
          const int a = cur[i - bpp], b = up ? up[i] : 0, c = up ? up[i - bpp] : 0;
          const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
          cur[i] = (unsigned char)(cur[i] + (pa <= pb && pa <= pc ? a : pb <= pc ? b : c));
        }
        break;
      default:
        return 1 + y;
    }
  }
  return 0;
}
