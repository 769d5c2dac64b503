// codec_san.cpp — the host encoders (vortex_amd/csrc/encode.cpp) and the oracle
// (oracle/vx_oracle.c) under -fsanitize=address,undefined: seeded random inputs of every shape
// the tests use (every ptype, empty and ragged lengths, all bit widths, patches, NaN/inf/-0.0
// floats, escapes) are encoded by vxe_* and decoded by vxo_*, and must round-trip bit-exactly;
// then the oracle's decoders that parse untrusted bytes (roaring, FSST codes, take indices,
// RunEnd ends) are fed garbage and must fail cleanly.  Test infrastructure (tests/
// test_sanitizers.py builds it with `make -C vortex_amd/csrc sanitize`); VERDICT r03 item 5.
// Usage: codec_san <iterations> <rng seed>  -> one JSON line of counts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/vortex_enc.h"
#include "../../oracle/vx_oracle.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

int g_fail = 0;
#define CHECK(cond, what)                                                                     \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "FAIL %s (line %d, iteration %llu)\n", what, __LINE__, it); \
            g_fail++;                                                                         \
        }                                                                                     \
    } while (0)

const int kU[4] = {0, 1, 2, 3};  // u8 u16 u32 u64 (VXG / VXO ptype ids)
const int kI[4] = {4, 5, 6, 7};  // i8 i16 i32 i64

uint64_t rand_len(Rng& r) {
    switch (r.below(5)) {
    case 0: return r.below(3);                 // 0, 1, 2
    case 1: return 1024 * (1 + r.below(3));    // whole blocks
    case 2: return 1023 + r.below(3);          // around a block edge
    default: return r.below(5000);
    }
}

void fill_ints(Rng& r, int w, uint64_t n, unsigned bits, std::vector<uint8_t>& out) {
    out.assign(size_t(n * w) + 8, 0);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t v = bits >= 64 ? r.next() : (r.next() & ((1ull << bits) - 1));
        if (r.below(50) == 0) v = r.next();  // outliers -> patches
        std::memcpy(out.data() + i * w, &v, size_t(w));
    }
}

void bitpack_roundtrip(Rng& r, unsigned long long it) {
    const int pt = kU[r.below(4)], w = vxo_ptype_width(pt), T = 8 * w;
    const uint64_t n = rand_len(r);
    std::vector<uint8_t> v;
    fill_ints(r, w, n, unsigned(r.below(T + 1)), v);
    const unsigned W = vxe_best_bit_width(pt, v.data(), n);
    CHECK(W <= unsigned(T), "best bit width <= T");
    std::vector<uint8_t> packed(size_t((n + 1023) / 1024) * 128 * (W ? W : 1) + 16);
    const uint64_t pb = vxe_bitpack(pt, W, v.data(), n, packed.data());
    std::vector<uint64_t> idx(n + 1);
    std::vector<uint8_t> pv(size_t(n * w) + 8);
    const uint64_t np = vxe_gather_patches(pt, W, v.data(), n, idx.data(), pv.data(), n + 1);
    std::vector<uint8_t> out(size_t(n * w) + 8, 0xCD);
    CHECK(vxo_unpack(pt, W, 0, n, packed.data(), pb, out.data()) == 0, "vxo_unpack");
    CHECK(vxo_patch(pt, out.data(), n, 3, idx.data(), 0, pv.data(), np) == 0, "vxo_patch");
    CHECK(std::memcmp(out.data(), v.data(), size_t(n * w)) == 0, "bitpack + patches round trip");
    if (n > 1 && W) {  // a slice inside the first block
        const unsigned off = unsigned(r.below(n < 1024 ? n : 1024));
        CHECK(vxo_unpack(pt, W, off, n - off, packed.data(), pb, out.data()) == 0, "vxo_unpack slice");
    }
}

void for_zigzag_roundtrip(Rng& r, unsigned long long it) {
    const bool sgn = r.below(2);
    const int k = int(r.below(4)), pt = sgn ? kI[k] : kU[k], w = vxo_ptype_width(pt);
    const uint64_t n = rand_len(r);
    std::vector<uint8_t> v;
    fill_ints(r, w, n, unsigned(r.below(8 * w + 1)), v);
    std::vector<uint8_t> enc(size_t(n * w) + 8), dec(size_t(n * w) + 8);
    uint64_t ref = 0;
    unsigned shift = 0;
    if (vxe_for_compress(pt, v.data(), n, enc.data(), &ref, &shift) == 0) {  // 1: a ConstantArray of zeros
        vxo_for_decode(pt, enc.data(), n, ref, shift, dec.data());
        CHECK(std::memcmp(dec.data(), v.data(), size_t(n * w)) == 0, "FoR round trip");
    }
    if (sgn) {
        vxe_zigzag_encode(pt, v.data(), n, enc.data());
        vxo_zigzag_decode(pt, enc.data(), n, dec.data());
        CHECK(std::memcmp(dec.data(), v.data(), size_t(n * w)) == 0, "ZigZag round trip");
    }
    // Delta: bases + deltas of whole 1024-value blocks (delta/compress.rs:100-166)
    if (n) {  // whole blocks + a scalar remainder
        std::vector<uint8_t> bases(size_t(n / 1024) * 128 + 16), deltas(size_t(n * w) + 8);
        vxe_delta_compress(kU[k], v.data(), n, bases.data(), deltas.data());
        const uint64_t nbases = (n / 1024) * (1024 / uint64_t(8 * w)) + (n % 1024 ? 1 : 0);
        const uint64_t off = r.below(n);
        CHECK(vxo_delta_decode(kU[k], bases.data(), nbases, deltas.data(), n, off, n - off, dec.data()) == 0,
              "delta decode");
        CHECK(std::memcmp(dec.data(), v.data() + off * w, size_t((n - off) * w)) == 0, "Delta round trip");
    }
}

template <class F, class I>
void alp_roundtrip(Rng& r, unsigned long long it) {
    const uint64_t n = rand_len(r);
    std::vector<F> v(n + 1);
    const int kind = int(r.below(3));
    for (uint64_t i = 0; i < n; i++) {
        double x = kind == 0 ? std::round(double(r.below(10000000)) ) / 100.0 : double(int64_t(r.next())) * 1e-9;
        if (r.below(40) == 0) {
            const double sp[] = {NAN, INFINITY, -INFINITY, -0.0, 1e300, 5e-324};
            x = sp[r.below(6)];
        }
        v[i] = F(x);
    }
    uint8_t e = 0, f = 0;
    std::vector<I> enc(n + 1);
    std::vector<uint64_t> pidx(n + 1);
    std::vector<F> pval(n + 1), out(n + 1);
    uint64_t np;
    if constexpr (sizeof(F) == 8) np = vxe_alp_encode_f64(v.data(), n, &e, &f, enc.data(), pidx.data(), pval.data(), n + 1);
    else np = vxe_alp_encode_f32(v.data(), n, &e, &f, enc.data(), pidx.data(), pval.data(), n + 1);
    if constexpr (sizeof(F) == 8) vxo_alp_decode_f64(enc.data(), n, e, f, out.data());
    else vxo_alp_decode_f32(enc.data(), n, e, f, out.data());
    CHECK(vxo_patch(sizeof(F) == 8 ? 3 : 2, out.data(), n, 3, pidx.data(), 0, pval.data(), np) == 0, "ALP patches");
    // bit-exact, except that -0.0 decodes as +0.0: the reference keeps a value unpatched when
    // decode(encode(v)) == v as floats (alp/mod.rs:191-197, `decoded != *v`), and -0.0 == 0.0
    bool alp_ok = true;
    for (uint64_t i = 0; i < n && alp_ok; i++)
        alp_ok = std::memcmp(&out[i], &v[i], sizeof(F)) == 0 || (v[i] == F(0) && out[i] == F(0));
    CHECK(alp_ok, "ALP round trip (bits; -0.0 -> +0.0 as the reference)");
    // ALP-RD
    uint8_t rbw = 0, dlen = 0;
    uint16_t dict[8] = {0};
    std::vector<uint16_t> left(n + 1), exc(n + 1);
    using R = std::conditional_t<sizeof(F) == 8, uint64_t, uint32_t>;
    std::vector<R> right(n + 1);
    std::vector<uint64_t> epos(n + 1);
    uint64_t ne;
    if constexpr (sizeof(F) == 8)
        ne = vxe_alprd_encode_f64(v.data(), n, &rbw, dict, &dlen, left.data(), right.data(), epos.data(), exc.data(), n + 1);
    else
        ne = vxe_alprd_encode_f32(v.data(), n, &rbw, dict, &dlen, left.data(), right.data(), epos.data(), exc.data(), n + 1);
    CHECK(dlen <= 8, "ALP-RD dictionary <= 8");
    if constexpr (sizeof(F) == 8)
        CHECK(vxo_alprd_decode_checked_f64(left.data(), dict, dlen, rbw, right.data(), n, epos.data(), exc.data(), ne, out.data()) == 0, "ALP-RD decode");
    else
        CHECK(vxo_alprd_decode_checked_f32(left.data(), dict, dlen, rbw, right.data(), n, epos.data(), exc.data(), ne, out.data()) == 0, "ALP-RD decode");
    CHECK(std::memcmp(out.data(), v.data(), size_t(n) * sizeof(F)) == 0, "ALP-RD round trip (bits)");
}

void dict_runend_roundtrip(Rng& r, unsigned long long it) {
    const int vws[] = {1, 2, 4, 8, 16};
    const int vw = vws[r.below(5)];
    const uint64_t n = rand_len(r), card = 1 + r.below(300);
    std::vector<uint8_t> pool(size_t(card * vw)), v(size_t(n * vw) + 16);
    for (auto& b : pool) b = uint8_t(r.next());
    uint64_t i = 0;
    while (i < n) {  // runs of 1..8 of one pool value
        const uint64_t c = r.below(card), len = 1 + r.below(8);
        for (uint64_t k = 0; k < len && i < n; k++, i++) std::memcpy(v.data() + i * vw, pool.data() + c * vw, size_t(vw));
    }
    std::vector<uint64_t> codes(n + 1);
    std::vector<uint8_t> dv(size_t((n + 1) * vw)), out(size_t(n * vw) + 16);
    const uint64_t nd = vxe_dict_encode(vw, v.data(), n, codes.data(), dv.data(), n + 1);
    CHECK(nd <= card, "dictionary size <= cardinality");
    CHECK(vxo_take(vw, dv.data(), nd, 3, codes.data(), n, out.data()) == 0, "take");
    CHECK(std::memcmp(out.data(), v.data(), size_t(n * vw)) == 0, "Dict round trip");
    std::vector<uint64_t> ends(n + 1);
    std::vector<uint8_t> rv(size_t((n + 1) * vw));
    const uint64_t nr = vxe_runend_encode(vw, v.data(), n, ends.data(), rv.data());
    if (n) {  // a slice: the runs from the first one ending past `off` (RunEndArray::slice)
        const uint64_t off = r.below(n), len = n - off;
        uint64_t r0 = 0;
        while (ends[r0] <= off) r0++;
        CHECK(vxo_runend_decode(vw, rv.data() + r0 * vw, 3, ends.data() + r0, nr - r0, off, len, out.data()) == 0,
              "RunEnd decode");
        CHECK(std::memcmp(out.data(), v.data() + off * vw, size_t(len * vw)) == 0, "RunEnd round trip");
    }
}

void fsst_roundtrip(Rng& r, unsigned long long it) {
    static const char* words[] = {"furiously", " regular", " deposits", " sleep", "carefully", " ", "the", "\xff\x01"};
    const uint64_t n = rand_len(r) % 2000;
    std::vector<uint8_t> heap;
    std::vector<int64_t> offs(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t parts = r.below(6);
        for (uint64_t p = 0; p < parts; p++) {
            if (r.below(10) == 0) {
                heap.push_back(uint8_t(r.next()));  // arbitrary bytes -> escapes
            } else {
                const char* w = words[r.below(8)];
                heap.insert(heap.end(), w, w + std::strlen(w));
            }
        }
        offs[i + 1] = int64_t(heap.size());
    }
    vxe_fsst_table t{};
    vxe_fsst_train(heap.data(), offs.data(), n, &t);
    CHECK(t.n_symbols <= 255, "<= 255 symbols");
    std::vector<uint8_t> codes(heap.size() * 2 + 16);
    std::vector<int32_t> coffs(n + 1);
    const uint64_t nc = vxe_fsst_compress(&t, heap.data(), offs.data(), n, codes.data(), codes.size(), coffs.data());
    CHECK(nc <= codes.size(), "codes fit");
    std::vector<int64_t> lens(n + 1);
    for (uint64_t i = 0; i < n; i++) lens[i] = offs[i + 1] - offs[i];
    std::vector<uint8_t> out(heap.size() + 16), views(size_t(n * 16) + 16);
    size_t hl = 0;
    CHECK(vxo_fsst_canonicalize(t.symbols, t.lens, codes.data(), 6, coffs.data(), 7, lens.data(), n, nullptr, out.data(),
                                &hl, views.data()) == 0,
          "FSST canonicalize");
    CHECK(hl == heap.size() && (heap.empty() || std::memcmp(out.data(), heap.data(), heap.size()) == 0),
          "FSST round trip");
}

void roaring_roundtrip(Rng& r, unsigned long long it) {
    const uint64_t len = r.below(4) == 0 ? 70000 + r.below(70000) : r.below(5000);
    std::vector<uint8_t> bits((len + 7) / 8 + 8, 0), out((len + 7) / 8 + 8, 0);
    const int mode = int(r.below(3));
    for (uint64_t i = 0; i < len; i++) {
        const bool b = mode == 0 ? r.below(2) : mode == 1 ? (i / 500) % 2 : r.below(100) == 0;
        if (b) bits[i / 8] |= uint8_t(1u << (i % 8));
    }
    std::vector<uint8_t> ser((len / 65536 + 1) * 8400 + 1024);  // a bitset container is 8 KiB
    const uint64_t sz = vxe_roaring_bool_encode(bits.data(), len, ser.data(), ser.size());
    CHECK(sz <= ser.size(), "roaring fits");
    CHECK(vxo_roaring_bool_decode(ser.data(), sz, len, out.data()) == 0, "roaring decode");
    CHECK(std::memcmp(out.data(), bits.data(), size_t(len / 8)) == 0, "roaring round trip");
}

// The oracle's parsers of untrusted bytes on garbage: a status, no out-of-bounds access.
void garbage(Rng& r, unsigned long long it) {
    const uint64_t n = r.below(300);
    std::vector<uint8_t> g(n + 1);
    for (auto& b : g) b = uint8_t(r.next());
    if (r.below(2) && n > 8) {  // a plausible cookie prefix
        const uint32_t cookie = r.below(2) ? 12346u : 12347u;
        std::memcpy(g.data(), &cookie, 4);
    }
    // exact-size copy so a read past the end is caught
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    if (n) std::memcpy(exact, g.data(), n);
    std::vector<uint8_t> bits(8192 + 8);
    (void)vxo_roaring_bool_decode(exact, n, 65536, bits.data());
    std::free(exact);
    // FSST codes over a random table: out sized as the contract says (8 bytes per code)
    uint64_t syms[255];
    uint8_t sl[255];
    for (int s = 0; s < 255; s++) {
        syms[s] = r.next();
        sl[s] = uint8_t(1 + r.below(8));
    }
    std::vector<uint8_t> out(8 * n + 16);
    (void)vxo_fsst_decompress(syms, sl, g.data(), n, out.data());
    // take with out-of-range codes -> -1
    std::vector<uint64_t> codes(n + 1);
    for (auto& c : codes) c = r.below(20);
    std::vector<uint8_t> vals(10 * 8), tk(8 * n + 8);
    const int tr = vxo_take(8, vals.data(), 10, 3, codes.data(), n, tk.data());
    bool any_oob = false;
    for (uint64_t i = 0; i < n; i++) any_oob |= codes[i] >= 10;
    CHECK((tr != 0) == any_oob, "take reports out-of-range codes");
    // RunEnd ends not covering the array -> -1, never a write past len
    std::vector<uint64_t> ends(8);
    for (auto& e : ends) e = r.below(100);
    std::vector<uint8_t> re(100 * 4 + 8);
    (void)vxo_runend_decode(4, vals.data(), 3, ends.data(), 8, 0, 100, re.data());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s iterations rng_seed\n", argv[0]);
        return 2;
    }
    const unsigned long long iters = std::strtoull(argv[1], nullptr, 10);
    Rng r{std::strtoull(argv[2], nullptr, 10) * 0x9E3779B97F4A7C15ull | 1};
    unsigned long long it = 0;
    for (it = 0; it < iters; it++) {
        bitpack_roundtrip(r, it);
        for_zigzag_roundtrip(r, it);
        if (it % 2 == 0) alp_roundtrip<double, int64_t>(r, it);
        else alp_roundtrip<float, int32_t>(r, it);
        dict_runend_roundtrip(r, it);
        if (it % 4 == 0) fsst_roundtrip(r, it);
        if (it % 4 == 1) roaring_roundtrip(r, it);
        garbage(r, it);
        if (g_fail > 20) break;
    }
    std::printf("{\"iterations\": %llu, \"failures\": %d}\n", it, g_fail);
    return g_fail ? 1 : 0;
}
