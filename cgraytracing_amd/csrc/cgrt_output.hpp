// Image output: the tone map of a finished image (cgrt_tonemap_rgb8; tonemap_byte itself stands beside the gather in
// cgrt_ppm_apply.hpp) and the PNG writer (cgrt_write_png).
// gammaCorr (util.h:45-47) and the vertical flip of main.cpp:403-412
__global__ void tonemap_kernel(const double *__restrict__ image, int W, int H, unsigned char *__restrict__ rgb8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // output byte index, top row first
    const long long n = (long long)W * H * 3;
    if (i >= n) return;
    const long long row = i / ((long long)W * 3), rest = i % ((long long)W * 3);
    rgb8[i] = tonemap_byte(image[(long long)(H - 1 - row) * W * 3 + rest]);
}

extern "C" int cgrt_tonemap_rgb8(int device, const double *image, int width, int height, uint8_t *rgb8) {
    if (!image || !rgb8 || width < 1 || height < 1) return fail(CGRT_ERR_INVALID, "bad argument");
    ON_DEVICE(device);
    const size_t n = (size_t)width * height * 3;
    DevBuf img, out;
    HIP_TRY(img.alloc(n * sizeof(double)));
    HIP_TRY(out.alloc(n));
    HIP_TRY(hipMemcpy(img.p, image, n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(tonemap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, img.as<double>(), width, height,
                       out.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rgb8, out.p, n, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// ---- PNG (host): signature, IHDR, one IDAT of stored deflate blocks, IEND -------------------------------------------
namespace {
struct Crc32 {
    uint32_t table[256];
    Crc32() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    }
    uint32_t run(uint32_t crc, const unsigned char *p, size_t n) const {
        for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
        return crc;
    }
};
void put32(std::vector<unsigned char> &v, uint32_t x) {
    v.push_back((unsigned char)(x >> 24)); v.push_back((unsigned char)(x >> 16));
    v.push_back((unsigned char)(x >> 8)); v.push_back((unsigned char)x);
}
bool write_chunk(FILE *f, const Crc32 &crc, const char type[4], const std::vector<unsigned char> &data) {
    std::vector<unsigned char> head;
    put32(head, (uint32_t)data.size());
    head.insert(head.end(), type, type + 4);
    uint32_t c = crc.run(0xffffffffu, head.data() + 4, 4);
    c = crc.run(c, data.data(), data.size()) ^ 0xffffffffu;
    std::vector<unsigned char> tail;
    put32(tail, c);
    return std::fwrite(head.data(), 1, head.size(), f) == head.size() &&
           (data.empty() || std::fwrite(data.data(), 1, data.size(), f) == data.size()) &&
           std::fwrite(tail.data(), 1, 4, f) == 4;
}
}  // namespace

extern "C" int cgrt_write_png(const char *path, int width, int height, const uint8_t *rgb8) {
    if (!path || !rgb8 || width < 1 || height < 1 || (uint64_t)width * height > (1ull << 28))
        return fail(CGRT_ERR_INVALID, "bad argument");
    // raw scanlines: filter byte 0 + width*3 bytes
    const size_t stride = (size_t)width * 3, raw_n = (stride + 1) * height;
    std::vector<unsigned char> raw(raw_n);
    for (int y = 0; y < height; y++) {
        raw[(stride + 1) * y] = 0;
        std::memcpy(&raw[(stride + 1) * y + 1], rgb8 + stride * y, stride);
    }
    std::vector<unsigned char> z;
    z.reserve(raw_n + raw_n / 65535 * 5 + 16);
    z.push_back(0x78); z.push_back(0x01);  // zlib header: deflate, 32 K window, no preset dictionary
    uint32_t a = 1, b = 0;                 // adler32
    for (size_t off = 0; off < raw_n; off += 65535) {
        const size_t len = raw_n - off < 65535 ? raw_n - off : 65535;
        z.push_back(off + len == raw_n ? 1 : 0);  // BFINAL, BTYPE = 00 (stored)
        z.push_back((unsigned char)(len & 0xff)); z.push_back((unsigned char)(len >> 8));
        z.push_back((unsigned char)(~len & 0xff)); z.push_back((unsigned char)((~len >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + len);
        for (size_t i = 0; i < len; i += 5552) {  // adler32 with deferred modulo
            const size_t m = len - i < 5552 ? len - i : 5552;
            for (size_t k = 0; k < m; k++) { a += raw[off + i + k]; b += a; }
            a %= 65521u; b %= 65521u;
        }
    }
    put32(z, (b << 16) | a);
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(CGRT_ERR_IO, std::string("cannot open ") + path);
    static const Crc32 crc;
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<unsigned char> ihdr;
    put32(ihdr, (uint32_t)width); put32(ihdr, (uint32_t)height);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);  // 8-bit RGB
    const bool ok = std::fwrite(sig, 1, 8, f) == 8 && write_chunk(f, crc, "IHDR", ihdr) && write_chunk(f, crc, "IDAT", z) &&
                    write_chunk(f, crc, "IEND", std::vector<unsigned char>());
    if (std::fclose(f) != 0 || !ok) return fail(CGRT_ERR_IO, std::string("write failed: ") + path);
    return CGRT_OK;
}
