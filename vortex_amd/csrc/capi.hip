// capi.hip — the C ABI (include/vortex_gpu.h): the context, the error text, options and launch
// statistics, memory and copy entry points, and the thin wrappers that construct a Planner
// (planner.hpp) or call a launcher.  The plan entry points are in plan.hip.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "encode_gpu.hpp"
#include "planner.hpp"

namespace vxg {

// ALP exponent tables (encodings/alp/src/alp/mod.rs:255-351).
const float kF10f[11] = {1.0f, 10.0f, 100.0f, 1000.0f, 10000.0f, 100000.0f, 1000000.0f,
                         10000000.0f, 100000000.0f, 1000000000.0f, 10000000000.0f};
const float kIF10f[11] = {1.0f, 0.1f, 0.01f, 0.001f, 0.0001f, 0.00001f, 0.000001f,
                          0.0000001f, 0.00000001f, 0.000000001f, 0.0000000001f};
const double kF10d[24] = {
    1.0, 10.0, 100.0, 1000.0, 10000.0, 100000.0, 1000000.0, 10000000.0, 100000000.0,
    1000000000.0, 10000000000.0, 100000000000.0, 1000000000000.0, 10000000000000.0,
    100000000000000.0, 1000000000000000.0, 10000000000000000.0, 100000000000000000.0,
    1000000000000000000.0, 10000000000000000000.0, 100000000000000000000.0,
    1000000000000000000000.0, 10000000000000000000000.0, 100000000000000000000000.0};
const double kIF10d[24] = {
    1.0, 0.1, 0.01, 0.001, 0.0001, 0.00001, 0.000001, 0.0000001, 0.00000001, 0.000000001,
    0.0000000001, 0.00000000001, 0.000000000001, 0.0000000000001, 0.00000000000001,
    0.000000000000001, 0.0000000000000001, 0.00000000000000001, 0.000000000000000001,
    0.0000000000000000001, 0.00000000000000000001, 0.000000000000000000001,
    0.0000000000000000000001, 0.00000000000000000000001};

static thread_local std::string g_last_error;

vxg_status set_error(vxg_status s, const std::string& msg) {
    if (s != VXG_OK) g_last_error = msg;
    return s;
}

vxg_status hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return VXG_OK;
    return set_error(e == hipErrorOutOfMemory ? VXG_ERR_OUT_OF_MEMORY : VXG_ERR_HIP,
                     std::string(what) + ": " + hipGetErrorString(e));
}

thread_local Ctx* g_cur_ctx = nullptr;

Options default_options() {
    static const Options d = [] {
        Options o;
        o.k1w_min_groups = int64_t(env_int("VXG_K1W_MIN_GROUPS", INT64_MIN, INT64_MAX, o.k1w_min_groups));
        return o;
    }();
    return d;
}

vxg_status use_device(vxg_ctx* ctx) {
    if (!ctx) return set_error(VXG_ERR_INVALID_ARGUMENT, "null vxg_ctx");
    g_cur_ctx = &ctx->c;  // this entry point's launches follow ctx's options
    return hip_check(hipSetDevice(ctx->c.device), "hipSetDevice");
}

// The device error word's bits -> the VortexError variant each one stands for.
vxg_status status_of_err_word(uint32_t err) {
    if (err & kErrTakeOOB) return set_error(VXG_ERR_OUT_OF_BOUNDS, "take: index out of bounds");
    if (err & kErrPatchOOB) return set_error(VXG_ERR_OUT_OF_BOUNDS, "patch index out of bounds");
    if (err & kErrPatchOrder) return set_error(VXG_ERR_INVALID_ARGUMENT, "patch indices are not sorted");
    if (err & kErrRunEnd) return set_error(VXG_ERR_INVALID_ARGUMENT, "RunEnd ends do not cover the array");
    if (err & kErrFsst) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST codes do not decode to uncompressed_lengths");
    if (err & kErrRoaring) return set_error(VXG_ERR_INVALID_SERDE, "RoaringBool buffer is not a croaring Native bitmap");
    if (err & kErrVarBin) return set_error(VXG_ERR_INVALID_ARGUMENT, "VarBin offsets out of range of the bytes");
    if (err & kErrPlanSync)
        return set_error(VXG_ERR_ASSERTION_FAILED, "plan launch: in-grid pre-pass records never published "
                                                   "(overlapping replays of one plan?)");
    return set_error(VXG_ERR_ASSERTION_FAILED, "unknown device error bit");
}

}  // namespace vxg

using namespace vxg;

// ===================================================================================
// C ABI
// ===================================================================================
// A value width a gather / broadcast kernel is instantiated for (16 = BinaryView rows).
static bool value_width_ok(unsigned vw) { return vw == 1 || vw == 2 || vw == 4 || vw == 8 || vw == 16; }

static const char* const kShiftRange = "FoR shift out of range";

static vxg_status bitunpack_common(vxg_ctx* ctx, int T, unsigned W, unsigned offset, uint64_t len,
                                   const void* packed, uint64_t packed_bytes, Epi epi, int vw,
                                   UnpackArgs a, void* out, void* stream) {
    if (a.shift >= unsigned(T)) return set_error(VXG_ERR_INVALID_ARGUMENT, kShiftRange);
    if (len && (!out || (W > 0 && !packed) || (epi == Epi::Dict && a.dict_len && !a.dict)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "null packed/dict/out");
    std::vector<K1Job> jobs(1);
    VXG_TRY(make_k1_job(T, W, offset, len, packed, packed_bytes, epi, vw, a, out, jobs[0]));
    return launch_k1_jobs(jobs, ctx->c.err_word, S(stream), nullptr, nullptr);
}

extern "C" {

int vxg_abi_version(void) { return VXG_ABI_VERSION; }

const char* vxg_last_error(void) { return g_last_error.c_str(); }

vxg_status vxg_open(int device, vxg_ctx** out) {
    if (!out) return set_error(VXG_ERR_INVALID_ARGUMENT, "null out");
    int n = 0;
    VXG_TRY(hip_check(hipGetDeviceCount(&n), "hipGetDeviceCount"));
    if (device < 0 || device >= n) return set_error(VXG_ERR_INVALID_ARGUMENT, "no such device");
    VXG_TRY(hip_check(hipSetDevice(device), "hipSetDevice"));
    auto* c = new vxg_ctx();
    c->c.device = device;
    c->c.opt = default_options();
    hipError_t e = hipMalloc(&c->c.err_word, 16);
    if (e == hipSuccess) e = hipMemset(c->c.err_word, 0, 16);
    if (e == hipSuccess) {
        // Planner temporaries come from the device's stream-ordered pool; keep freed blocks
        // cached instead of returning them to the driver at every synchronisation (the default
        // threshold 0 made each canonicalize re-map its temporaries: ~25 us of host time).
        hipMemPool_t pool;
        uint64_t keep = ~0ull;
        if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess)
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    if (e == hipSuccess) e = fsst_diag_init();  // (a synchronous copy: never inside a plan's capture)
    if (e != hipSuccess) {
        vxg_close(c);
        return hip_check(e, "context setup");
    }
    *out = c;
    return VXG_OK;
}

vxg_status vxg_set_option(vxg_ctx* ctx, int option, int64_t value) {
    if (!ctx) return set_error(VXG_ERR_INVALID_ARGUMENT, "null vxg_ctx");
    Options& o = ctx->c.opt;
    switch (option) {
    case VXG_OPT_K1W_MIN_GROUPS:
        if (value < 0 || value > (int64_t(1) << 31)) return set_error(VXG_ERR_INVALID_ARGUMENT, "K1W_MIN_GROUPS out of range");
        o.k1w_min_groups = value;
        return VXG_OK;
    case VXG_OPT_K1W_BPW:
        if (value < 0 || value > 32) return set_error(VXG_ERR_INVALID_ARGUMENT, "K1W_BPW must be in [0, 32]");
        o.k1w_bpw = value;
        return VXG_OK;
    case VXG_OPT_K1_WAVE:
        if (value < -1 || value > 2) return set_error(VXG_ERR_INVALID_ARGUMENT, "K1_WAVE must be -1, 0, 1 or 2");
        o.k1_wave = value;
        return VXG_OK;
    }
    return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown option " + std::to_string(option));
}

vxg_status vxg_get_option(vxg_ctx* ctx, int option, int64_t* value) {
    if (!ctx || !value) return set_error(VXG_ERR_INVALID_ARGUMENT, "null argument");
    const Options& o = ctx->c.opt;
    switch (option) {
    case VXG_OPT_K1W_MIN_GROUPS: *value = o.k1w_min_groups; return VXG_OK;
    case VXG_OPT_K1W_BPW: *value = o.k1w_bpw; return VXG_OK;
    case VXG_OPT_K1_WAVE: *value = o.k1_wave; return VXG_OK;
    }
    return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown option " + std::to_string(option));
}

vxg_status vxg_get_launch_stats(vxg_ctx* ctx, vxg_launch_stats* out, int reset) {
    if (!ctx || !out) return set_error(VXG_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    const LaunchStats& st = ctx->c.st;
    *out = vxg_launch_stats{};
    out->k1w_launches = st.k1w_launches;
    out->k1w_last_groups = st.k1w_last_groups;
    out->k1w_last_bpw = st.k1w_last_bpw;
    out->k1w_min_bpw = st.k1w_min_bpw;
    out->k1w_max_bpw = st.k1w_max_bpw;
    out->k1w_last_bpw_max = st.k1w_last_bpw_max;
    if (reset) ctx->c.st = LaunchStats{};
    return VXG_OK;
}

vxg_status vxg_close(vxg_ctx* ctx) {
    if (!ctx) return VXG_OK;
    if (g_cur_ctx == &ctx->c) g_cur_ctx = nullptr;
    (void)hipSetDevice(ctx->c.device);
    (void)hipDeviceSynchronize();
    if (ctx->c.err_word) (void)hipFree(ctx->c.err_word);
    delete ctx;
    return VXG_OK;
}

vxg_status vxg_alloc(vxg_ctx* ctx, uint64_t bytes, void** dptr) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipMalloc(dptr, bytes ? bytes : 16), "hipMalloc");
}

vxg_status vxg_free(vxg_ctx* ctx, void* dptr) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipFree(dptr), "hipFree");
}

vxg_status vxg_host_alloc(vxg_ctx* ctx, uint64_t bytes, void** hptr) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipHostMalloc(hptr, bytes ? bytes : 16, hipHostMallocDefault), "hipHostMalloc");
}

vxg_status vxg_host_free(vxg_ctx* ctx, void* hptr) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipHostFree(hptr), "hipHostFree");
}

vxg_status vxg_memcpy_h2d(vxg_ctx* ctx, void* dst, const void* src, uint64_t bytes, void* stream) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)), "h2d");
}

vxg_status vxg_memcpy_d2h(vxg_ctx* ctx, void* dst, const void* src, uint64_t bytes, void* stream) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)), "d2h");
}

vxg_status vxg_memcpy_d2d(vxg_ctx* ctx, void* dst, const void* src, uint64_t bytes, void* stream) {
    VXG_TRY(use_device(ctx));
    return hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(stream)), "d2d");
}

vxg_status vxg_stream_sync(vxg_ctx* ctx, void* stream) {
    VXG_TRY(use_device(ctx));
    VXG_TRY(hip_check(hipStreamSynchronize(S(stream)), "hipStreamSynchronize"));
    uint32_t err = 0;
    VXG_TRY(hip_check(hipMemcpy(&err, ctx->c.err_word, 4, hipMemcpyDeviceToHost), "error word readback"));
    if (err) {
        VXG_TRY(hip_check(hipMemset(ctx->c.err_word, 0, 4), "error word reset"));
        return status_of_err_word(err);
    }
    return VXG_OK;
}

vxg_status vxg_canonical_size(vxg_ctx* ctx, const vxg_array* a, uint64_t* values_bytes, uint64_t* data_bytes) {
    VXG_TRY(use_device(ctx));
    if (!a) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array");
    Planner p(ctx, nullptr);
    p.as_query();
    uint64_t vb = 0, db = 0;
    VXG_TRY(p.canonical_size(*a, vb, db));
    if (values_bytes) *values_bytes = vb;
    if (data_bytes) *data_bytes = db;
    return VXG_OK;
}

vxg_status vxg_canonical_layout(vxg_ctx* ctx, const vxg_array* a, uint64_t* values_bytes, uint64_t* data_bytes,
                                vxg_data_buffer* bufs, uint32_t cap, uint32_t* n_bufs) {
    VXG_TRY(use_device(ctx));
    if (!a) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array");
    Planner p(ctx, nullptr);
    p.as_query();
    uint64_t vb = 0, db = 0;
    uint32_t n = 0;
    if (is_string(*a)) {
        std::vector<vxg_data_buffer> v;
        VXG_TRY(p.string_layout(*a, v, db));
        vb = 16 * a->len;
        n = uint32_t(v.size());
        if (bufs && cap < n) return set_error(VXG_ERR_INVALID_ARGUMENT, "buffer table too small");
        if (bufs) std::copy(v.begin(), v.end(), bufs);
    } else {
        VXG_TRY(p.canonical_size(*a, vb, db));
    }
    if (values_bytes) *values_bytes = vb;
    if (data_bytes) *data_bytes = db;
    if (n_bufs) *n_bufs = n;
    return VXG_OK;
}

vxg_status vxg_canonicalize(vxg_ctx* ctx, const vxg_array* a, vxg_canonical* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!a || !out) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array/out");
    Planner p(ctx, S(stream));
    return p.canonical(*a, *out);
}

static int unsigned_T(int ptype) { return 8 * ptype_width(ptype); }

vxg_status vxg_bitunpack(vxg_ctx* ctx, int ptype, unsigned bit_width, unsigned offset, uint64_t len,
                         const void* packed, uint64_t packed_bytes, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "BitPacked needs an integer ptype");
    return bitunpack_common(ctx, unsigned_T(ptype), bit_width, offset, len, packed, packed_bytes, Epi::Plain, 0,
                            UnpackArgs{}, out, stream);
}

vxg_status vxg_bitunpack_for(vxg_ctx* ctx, int ptype, unsigned bit_width, unsigned offset, uint64_t len,
                             const void* packed, uint64_t packed_bytes, uint64_t reference, unsigned shift,
                             int zigzag, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "FoR needs an integer ptype");
    UnpackArgs a{};
    a.reference = reference;
    a.shift = shift;
    return bitunpack_common(ctx, unsigned_T(ptype), bit_width, offset, len, packed, packed_bytes,
                            zigzag ? Epi::ForZigZag : Epi::For, 0, a, out, stream);
}

vxg_status vxg_bitunpack_alp(vxg_ctx* ctx, int float_ptype, unsigned bit_width, unsigned offset, uint64_t len,
                             const void* packed, uint64_t packed_bytes, uint64_t for_reference,
                             unsigned for_shift, unsigned e, unsigned f, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    const bool f32 = float_ptype == VXG_F32;
    if (!f32 && float_ptype != VXG_F64) return set_error(VXG_ERR_MISMATCHED_TYPES, "ALP decodes to f32/f64");
    if ((f32 && (e > 10 || f > 10)) || (!f32 && (e > 23 || f > 23)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "ALP exponents out of range");
    UnpackArgs a{};
    a.reference = for_reference;
    a.shift = for_shift;
    a.alp_a = f32 ? double(kF10f[f]) : kF10d[f];
    a.alp_b = f32 ? double(kIF10f[e]) : kIF10d[e];
    return bitunpack_common(ctx, f32 ? 32 : 64, bit_width, offset, len, packed, packed_bytes,
                            f32 ? Epi::AlpF32 : Epi::AlpF64, 0, a, out, stream);
}

vxg_status vxg_bitunpack_dict(vxg_ctx* ctx, int codes_ptype, unsigned bit_width, unsigned offset, uint64_t len,
                              const void* packed, uint64_t packed_bytes, const void* dict_values,
                              uint64_t dict_len, unsigned value_width, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_unsigned(codes_ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "Dict codes must be unsigned");
    if (!value_width_ok(value_width)) return set_error(VXG_ERR_INVALID_ARGUMENT, "value width must be 1, 2, 4, 8 or 16");
    if (bit_width > unsigned(kDictFusedMaxW))
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "fused dict decode supports code widths <= 16");
    UnpackArgs a{};
    a.dict = dict_values;
    a.dict_len = dict_len;
    return bitunpack_common(ctx, unsigned_T(codes_ptype), bit_width, offset, len, packed, packed_bytes, Epi::Dict,
                            int(value_width), a, out, stream);
}

vxg_status vxg_bitunpack_dict_chunks(vxg_ctx* ctx, int codes_ptype, unsigned bit_width, unsigned value_width,
                                     const vxg_dict_chunk* chunks_host, uint32_t n_chunks, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_unsigned(codes_ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "Dict codes must be unsigned");
    if (!value_width_ok(value_width)) return set_error(VXG_ERR_INVALID_ARGUMENT, "value width must be 1, 2, 4, 8 or 16");
    if (bit_width > unsigned(kDictFusedMaxW))
        return set_error(VXG_ERR_NOT_IMPLEMENTED, "fused dict decode supports code widths <= 16");
    if (n_chunks && !chunks_host) return set_error(VXG_ERR_INVALID_ARGUMENT, "null chunk table");
    std::vector<K1Job> jobs(n_chunks);
    for (uint32_t i = 0; i < n_chunks; i++) {
        const vxg_dict_chunk& c = chunks_host[i];
        if (c.n_blocks != (c.len + 1023) / 1024)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "chunk n_blocks != ceil(len/1024)");
        if (c.len && (!c.out || (bit_width > 0 && !c.packed) || (c.dict_len && !c.dict_values)))
            return set_error(VXG_ERR_INVALID_ARGUMENT, "null packed/dict/out in a chunk");
        UnpackArgs a{};
        a.dict = c.dict_values;
        a.dict_len = c.dict_len;
        VXG_TRY(make_k1_job(unsigned_T(codes_ptype), bit_width, 0, c.len, c.packed, c.n_blocks * 128ull * bit_width,
                            Epi::Dict, int(value_width), a, c.out, jobs[i]));
    }
    return launch_k1_jobs(jobs, ctx->c.err_word, S(stream), nullptr, nullptr);
}

vxg_status vxg_patch(vxg_ctx* ctx, int ptype, void* out, uint64_t out_len, int indices_ptype, const void* indices,
                     uint64_t indices_offset, const void* values, uint64_t n_patches, void* stream) {
    VXG_TRY(use_device(ctx));
    const int w = ptype_width(ptype);
    if (!w || !ptype_is_int(indices_ptype)) return set_error(VXG_ERR_INVALID_ARGUMENT, "bad ptype");
    if (n_patches && (!out || !indices || !values)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null out/indices/values");
    UnpackArgs a{};
    a.err = ctx->c.err_word;
    IntCol ic{};
    ic.p = indices;
    ic.width = ptype_width(indices_ptype);
    ic.sgn = ptype_is_signed(indices_ptype);
    return launch_patch(0, ic, Epi::Plain, 8 * w, out, out_len, indices_offset, values, n_patches, a, S(stream));
}

vxg_status vxg_for_decode(vxg_ctx* ctx, int ptype, const void* in, uint64_t n, uint64_t reference,
                          unsigned shift, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "FoR needs an integer ptype");
    if (shift >= unsigned(8 * ptype_width(ptype))) return set_error(VXG_ERR_INVALID_ARGUMENT, kShiftRange);
    if (n && (!in || !out)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null in/out");
    return launch_for(ptype_width(ptype), in, n, reference, shift, false, out, S(stream));
}

vxg_status vxg_zigzag_decode(vxg_ctx* ctx, int out_ptype, const void* in, uint64_t n, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_signed(out_ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "ZigZag decodes to signed ints");
    if (n && (!in || !out)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null in/out");
    return launch_zigzag(ptype_width(out_ptype), in, n, out, S(stream));
}

vxg_status vxg_alp_decode(vxg_ctx* ctx, int float_ptype, const void* encoded, uint64_t n, unsigned e, unsigned f,
                          void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    const bool f32 = float_ptype == VXG_F32;
    if (!f32 && float_ptype != VXG_F64) return set_error(VXG_ERR_MISMATCHED_TYPES, "ALP decodes to f32 or f64 only");
    if ((f32 && (e > 10 || f > 10)) || (!f32 && (e > 23 || f > 23)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "ALP exponents out of range");
    if (n && (!encoded || !out)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null encoded/out");
    return launch_alp(float_ptype, encoded, n, f32 ? double(kF10f[f]) : kF10d[f],
                      f32 ? double(kIF10f[e]) : kIF10d[e], out, S(stream));
}

vxg_status vxg_alprd_decode(vxg_ctx* ctx, int float_ptype, const uint16_t* left_codes, const uint16_t* dict_host,
                            unsigned dict_len, unsigned right_bw, const void* right, uint64_t n,
                            const uint64_t* exc_pos, const uint16_t* exc_vals, uint64_t n_exc, void* out,
                            void* stream) {
    VXG_TRY(use_device(ctx));
    if (float_ptype != VXG_F32 && float_ptype != VXG_F64)
        return set_error(VXG_ERR_MISMATCHED_TYPES, "ALP-RD decodes to f32 or f64 only");
    if (dict_len > 8) return set_error(VXG_ERR_INVALID_ARGUMENT, "ALP-RD dictionary holds at most 8 entries");
    if (right_bw == 0 || right_bw >= (float_ptype == VXG_F32 ? 32u : 64u))  // the left part is shifted by it
        return set_error(VXG_ERR_INVALID_ARGUMENT, "ALP-RD right bit width (shift) out of range");
    if ((dict_len && !dict_host) || (n && (!left_codes || !right || !out)) || (n_exc && (!exc_pos || !exc_vals)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "null dict/left/right/exceptions/out");
    return launch_alprd(float_ptype, left_codes, dict_host, dict_len, right_bw, right, n, exc_pos, 8, false, 0,
                        exc_vals, n_exc, out, ctx->c.err_word, S(stream));
}

vxg_status vxg_take(vxg_ctx* ctx, unsigned value_width, const void* values, uint64_t n_values, int codes_ptype,
                    const void* codes, uint64_t n, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_unsigned(codes_ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "take indices must be unsigned");
    if (!value_width_ok(value_width)) return set_error(VXG_ERR_INVALID_ARGUMENT, "value width must be 1, 2, 4, 8 or 16");
    if (n && (!codes || !out || (n_values && !values))) return set_error(VXG_ERR_INVALID_ARGUMENT, "null values/codes/out");
    return launch_take(int(value_width), values, n_values, ptype_width(codes_ptype), ptype_is_signed(codes_ptype), codes, n, out,
                       ctx->c.err_word, S(stream));
}

vxg_status vxg_delta_decode(vxg_ctx* ctx, int ptype, const void* bases, uint64_t n_bases, const void* deltas,
                            uint64_t n_deltas, uint64_t offset, uint64_t len, void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    const int w = ptype_width(ptype);
    if (!ptype_is_unsigned(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "Delta decodes unsigned ints");
    const uint64_t lanes = 1024 / (8 * w);
    if (n_bases != (n_deltas / 1024) * lanes + (n_deltas % 1024 ? 1 : 0))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "DeltaArray: bases.len() != expected_bases_len");
    if (offset > n_deltas || len > n_deltas - offset) return set_error(VXG_ERR_INVALID_ARGUMENT, "offset + len > deltas len");
    if (len == 0) return VXG_OK;
    if (!bases || !deltas || !out) return set_error(VXG_ERR_INVALID_ARGUMENT, "null bases/deltas/out");
    return launch_delta(w, bases, deltas, n_deltas, offset, len, out, S(stream));
}

vxg_status vxg_runend_decode(vxg_ctx* ctx, unsigned value_width, const void* values, int ends_ptype,
                             const void* ends, uint64_t n_runs, uint64_t offset, uint64_t len, void* out,
                             void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(ends_ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "RunEnd ends must be integers");
    if (!value_width_ok(value_width)) return set_error(VXG_ERR_INVALID_ARGUMENT, "value width must be 1, 2, 4, 8 or 16");
    if (len && n_runs && (!values || !ends || !out)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null values/ends/out");
    RunEndChunk c{};
    c.ends.p = ends;
    c.ends.width = ptype_width(ends_ptype);
    c.ends.sgn = ptype_is_signed(ends_ptype);
    c.values.p = values;
    c.values.width = int(value_width);
    c.out = out;
    c.n_runs = n_runs;
    c.offset = offset;
    c.len = len;
    return launch_runend(int(value_width), c, ctx->c.err_word, S(stream));
}

vxg_status vxg_take_array_ex(vxg_ctx* ctx, const vxg_array* a, int indices_ptype, const void* indices,
                             uint64_t n_indices, uint32_t flags, vxg_canonical* out, vxg_take_info* info,
                             void* stream) {
    VXG_TRY(use_device(ctx));
    if (!a || !out || (n_indices && !indices)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array/indices/out");
    if (!ptype_is_int(indices_ptype)) return set_error(VXG_ERR_INVALID_ARGUMENT, "take indices must be integers");
    vxg_take_info ti{};
    Planner p(ctx, S(stream));
    void* const in[4] = {out->values, out->validity, out->views, out->data};
    const vxg_status st =
        p.take(*a, indices, ptype_width(indices_ptype), ptype_is_signed(indices_ptype), n_indices, flags, *out, ti);
    if (info) *info = ti;
    if (st != VXG_OK) {  // nothing engine-allocated is handed back with an error
        void** const cur[4] = {&out->values, &out->validity, &out->views, &out->data};
        for (int i = 0; i < 4; i++) {
            if (*cur[i] && *cur[i] != in[i]) (void)hipFree(*cur[i]);
            *cur[i] = in[i];
        }
    }
    return st;
}

vxg_status vxg_take_array(vxg_ctx* ctx, const vxg_array* a, int indices_ptype, const void* indices,
                          uint64_t n_indices, vxg_canonical* out, void* stream) {
    return vxg_take_array_ex(ctx, a, indices_ptype, indices, n_indices, 0, out, nullptr, stream);
}

vxg_status vxg_compare_scalar(vxg_ctx* ctx, const vxg_array* a, int op, const void* scalar_host, uint32_t flags,
                              vxg_canonical* out, vxg_compare_info* info, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!a || !out || !scalar_host) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array/scalar/out");
    uint64_t bits = 0;  // the scalar's little-endian bytes (a->ptype's width; checked by the planner)
    if (a->dtype == VXG_DTYPE_PRIMITIVE) std::memcpy(&bits, scalar_host, size_t(ptype_width(a->ptype)));
    vxg_compare_info ci{};
    Planner p(ctx, S(stream));
    void* const values_in = out->values;
    void* const validity_in = out->validity;
    const vxg_status st = p.compare(*a, op, bits, flags, *out, ci);
    if (info) *info = ci;
    if (st != VXG_OK) {  // nothing engine-allocated is handed back with an error
        if (out->values && out->values != values_in) (void)hipFree(out->values);
        if (out->validity && out->validity != validity_in) (void)hipFree(out->validity);
        out->values = values_in;
        out->validity = validity_in;
    }
    return st;
}

vxg_status vxg_compare_bytes(vxg_ctx* ctx, const vxg_array* a, int op, const void* scalar_host, uint64_t scalar_len,
                             uint32_t flags, vxg_canonical* out, vxg_compare_bytes_info* info, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!a || !out || (scalar_len && !scalar_host)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array/scalar/out");
    vxg_compare_bytes_info ci{};
    Planner p(ctx, S(stream));
    void* const values_in = out->values;
    void* const validity_in = out->validity;
    const vxg_status st = p.compare_bytes(*a, op, scalar_host, scalar_len, flags, *out, ci);
    if (info) *info = ci;
    if (st != VXG_OK) {  // nothing engine-allocated is handed back with an error
        if (out->values && out->values != values_in) (void)hipFree(out->values);
        if (out->validity && out->validity != validity_in) (void)hipFree(out->validity);
        out->values = values_in;
        out->validity = validity_in;
    }
    return st;
}

vxg_status vxg_row_filter(vxg_ctx* ctx, const vxg_predicate* preds, uint32_t n_preds, uint32_t flags, vxg_canonical* out,
                          uint64_t* true_count_dev, vxg_row_filter_info* info, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!preds || !out || n_preds == 0) return set_error(VXG_ERR_INVALID_ARGUMENT, "row filter: null preds/out or no conjunct");
    const uint32_t both = VXG_ROWF_FUSE_RANGES | VXG_ROWF_NO_FUSE_RANGES;
    if ((flags & ~both) || (flags & both) == both) return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown row filter flags");
    if (reinterpret_cast<uintptr_t>(true_count_dev) & 7)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "row filter true count must be 8-byte aligned");
    for (uint32_t i = 0; i < n_preds; i++) {  // every conjunct, before anything is launched or allocated
        const vxg_predicate& p = preds[i];
        const std::string at = "row filter conjunct " + std::to_string(i);
        if (!p.column) return set_error(VXG_ERR_INVALID_ARGUMENT, at + ": null column");
        if (p.reserved) return set_error(VXG_ERR_INVALID_ARGUMENT, at + ": reserved must be 0");
        if (p.op < VXG_CMP_EQ || p.op > VXG_CMP_LTE)
            return set_error(VXG_ERR_INVALID_ARGUMENT, at + ": unknown compare operator " + std::to_string(p.op));
        if (p.column->len != preds[0].column->len)
            return set_error(VXG_ERR_INVALID_ARGUMENT, "Boolean operations aren't supported on arrays of different lengths");
        if (p.column->dtype == VXG_DTYPE_PRIMITIVE) {
            if (ptype_width(p.column->ptype) == 0 || p.column->ptype == VXG_F16)
                return set_error(VXG_ERR_NOT_IMPLEMENTED, at + ": compare does not support f16");
            if (!p.scalar_host) return set_error(VXG_ERR_INVALID_ARGUMENT, at + ": null scalar");
        } else if (is_string(*p.column)) {
            if (p.scalar_len && !p.scalar_host) return set_error(VXG_ERR_INVALID_ARGUMENT, at + ": null scalar");
        } else if (p.column->dtype == VXG_DTYPE_BOOL) {
            return set_error(VXG_ERR_NOT_IMPLEMENTED, at + ": Bool columns are not supported");
        } else {
            return set_error(VXG_ERR_MISMATCHED_TYPES, at + ": expected a primitive, utf8 or binary column");
        }
    }
    vxg_row_filter_info ri{};
    Planner p(ctx, S(stream));
    const vxg_canonical in = *out;
    const vxg_status st = p.row_filter(preds, n_preds, flags, *out, true_count_dev, ri);
    if (info) *info = ri;
    if (st != VXG_OK) {  // nothing engine-allocated is handed back with an error
        if (out->values && out->values != in.values) (void)hipFree(out->values);
        *out = in;
    }
    return st;
}

// ---- encoders on the GPU (encode_gpu.hip, fl_pack_impl.hpp) ----------------------------
vxg_status vxg_compute_int_stats(vxg_ctx* ctx, int ptype, const void* values, uint64_t n, vxg_int_stats* out,
                                 void* stream) {
    VXG_TRY(use_device(ctx));
    if (!out || (n && !values)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null values/out");
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "integer statistics need an integer ptype");
    IntStats st{};
    VXG_TRY(launch_int_stats(ptype_width(ptype), ptype_is_signed(ptype), values, n, &st, S(stream)));
    std::memset(out, 0, sizeof(*out));
    out->n = st.n;
    out->min_bits = st.min_bits;
    out->max_bits = st.max_bits;
    out->trailing_zeros = st.trailing_zeros;
    std::memcpy(out->bit_width_freq, st.bit_width_freq, sizeof(out->bit_width_freq));
    return VXG_OK;
}

static vxg_status pack_common(vxg_ctx* ctx, int ptype, bool for_, uint64_t reference, unsigned shift,
                              unsigned bit_width, const void* values, uint64_t n, void* packed, uint64_t packed_bytes,
                              void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "bitpack needs an integer ptype");
    const int T = 8 * ptype_width(ptype);
    if (bit_width >= unsigned(T))  // bitpack_encode (bitpacking/compress.rs:22-30)
        return set_error(VXG_ERR_INVALID_ARGUMENT,
                         "Cannot pack -- specified bit width is greater than or equal to raw bit width");
    const uint64_t want = ((n + 1023) / 1024) * 128ull * bit_width;
    if (packed_bytes != want)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "packed buffer must hold " + std::to_string(want) + " bytes");
    if (bit_width == 0 || n == 0) return VXG_OK;  // bit width 0: an empty buffer (compress.rs:86-88)
    if (!values || !packed) return set_error(VXG_ERR_INVALID_ARGUMENT, "null values/packed");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return set_error(VXG_ERR_INVALID_ARGUMENT, "packed must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(values) % uint64_t(ptype_width(ptype)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "values must be aligned to the value width");
    const bool sgn = ptype_is_signed(ptype);
    switch (T) {
    case 8: return fl_pack_8(int(bit_width), for_, reference, shift, sgn, values, n, packed, S(stream));
    case 16: return fl_pack_16(int(bit_width), for_, reference, shift, sgn, values, n, packed, S(stream));
    case 32: return fl_pack_32(int(bit_width), for_, reference, shift, sgn, values, n, packed, S(stream));
    default: return fl_pack_64(int(bit_width), for_, reference, shift, sgn, values, n, packed, S(stream));
    }
}

vxg_status vxg_bitpack(vxg_ctx* ctx, int ptype, unsigned bit_width, const void* values, uint64_t n, void* packed,
                       uint64_t packed_bytes, void* stream) {
    return pack_common(ctx, ptype, false, 0, 0, bit_width, values, n, packed, packed_bytes, stream);
}

vxg_status vxg_for_bitpack(vxg_ctx* ctx, int ptype, uint64_t reference, unsigned shift, unsigned bit_width,
                           const void* values, uint64_t n, void* packed, uint64_t packed_bytes, void* stream) {
    if (shift >= unsigned(8 * ptype_width(ptype))) return set_error(VXG_ERR_INVALID_ARGUMENT, "FoR shift out of range");
    return pack_common(ctx, ptype, true, reference, shift, bit_width, values, n, packed, packed_bytes, stream);
}

vxg_status vxg_for_encode(vxg_ctx* ctx, int ptype, const void* values, uint64_t n, uint64_t reference, unsigned shift,
                          void* out, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "FoR needs an integer ptype");
    if (shift >= unsigned(8 * ptype_width(ptype))) return set_error(VXG_ERR_INVALID_ARGUMENT, "FoR shift out of range");
    if (n && (!values || !out)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null values/out");
    if (n == 0) return VXG_OK;
    return launch_for_encode(ptype_width(ptype), ptype_is_signed(ptype), values, n, reference, shift, out, S(stream));
}

vxg_status vxg_gather_patches(vxg_ctx* ctx, int ptype, unsigned bit_width, const void* values, uint64_t n,
                              uint64_t* indices, void* patch_values, uint64_t cap, uint64_t* n_patches, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!n_patches || (n && !values) || (cap && (!indices || !patch_values)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "null argument");
    if (!ptype_is_int(ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "patches need an integer ptype");
    return launch_gather_patches_gpu(ptype_width(ptype), bit_width, values, n, indices, patch_values, cap, n_patches,
                                     S(stream));
}

vxg_status vxg_alp_encode(vxg_ctx* ctx, int float_ptype, const void* values, uint64_t n, uint8_t* e, uint8_t* f,
                          void* encoded, uint64_t* patch_indices, void* patch_values, uint64_t cap,
                          uint64_t* n_patches, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!e || !f || !n_patches || (n && (!values || !encoded)) || (cap && (!patch_indices || !patch_values)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "null argument");
    return launch_alp_encode(float_ptype, values, n, e, f, encoded, patch_indices, patch_values, cap, n_patches,
                             S(stream));
}

vxg_status vxg_fsst_compress(vxg_ctx* ctx, const uint64_t* symbols, const uint8_t* symbol_lengths, uint32_t n_symbols,
                             int offsets_ptype, const void* offsets, const uint8_t* bytes, uint64_t bytes_len,
                             const uint8_t* validity, uint64_t n, uint8_t* codes, uint64_t codes_cap,
                             int32_t* code_offsets, int32_t* uncompressed_lengths, uint64_t* codes_len, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!codes_len || !code_offsets || (n_symbols && (!symbols || !symbol_lengths)) ||
        (n && (!offsets || !uncompressed_lengths)) || (bytes_len && !bytes) || (codes_cap && !codes))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "null argument");
    if (!ptype_is_int(offsets_ptype)) return set_error(VXG_ERR_MISMATCHED_TYPES, "VarBin offsets must be integers");
    return launch_fsst_compress(symbols, symbol_lengths, n_symbols, ptype_width(offsets_ptype),
                                ptype_is_signed(offsets_ptype), offsets, bytes, bytes_len, validity, n, codes, codes_cap,
                                code_offsets, uncompressed_lengths, codes_len, S(stream));
}

vxg_status vxg_filter_array(vxg_ctx* ctx, const vxg_array* a, const vxg_array* predicate, vxg_canonical* out,
                            void* stream) {
    VXG_TRY(use_device(ctx));
    if (!a || !predicate || !out) return set_error(VXG_ERR_INVALID_ARGUMENT, "null array/predicate/out");
    vxg_status st;
    {
        Planner p(ctx, S(stream));
        st = p.filter(*a, *predicate, *out);
    }
    if (st != VXG_OK) return st;
    // synchronous like the reference's compute::filter: every output is complete on return
    return hip_check(hipStreamSynchronize(S(stream)), "filter sync");
}

vxg_status vxg_filter_batch(vxg_ctx* ctx, const vxg_array* const* columns, uint32_t n_columns, const void* mask,
                            uint64_t len, uint32_t flags, vxg_canonical* outs, uint64_t* true_count,
                            vxg_filter_batch_info* info, void* stream) {
    VXG_TRY(use_device(ctx));
    if (n_columns == 0 || !columns || !outs)
        return set_error(VXG_ERR_INVALID_ARGUMENT, "filter batch: null columns/outs or no column");
    if (len && !mask) return set_error(VXG_ERR_INVALID_ARGUMENT, "filter batch: null mask");
    if (reinterpret_cast<uintptr_t>(mask) & 7) return set_error(VXG_ERR_INVALID_ARGUMENT, "filter batch: mask must be 8-byte aligned");
    if (flags & ~uint32_t(VXG_FILTB_CANONICALIZE)) return set_error(VXG_ERR_INVALID_ARGUMENT, "unknown filter batch flags");
    for (uint32_t i = 0; i < n_columns; i++) {  // every column, before anything is launched or allocated
        const vxg_array* a = columns[i];
        if (!a) return set_error(VXG_ERR_INVALID_ARGUMENT, "filter batch column " + std::to_string(i) + ": null column");
        if (a->len != len)  // filter.rs:33-39
            return set_error(VXG_ERR_INVALID_ARGUMENT, "predicate.len() is " + std::to_string(len) +
                                                           ", does not equal array.len() of " + std::to_string(a->len));
        if (!is_string(*a) && a->dtype != VXG_DTYPE_BOOL && a->dtype != VXG_DTYPE_PRIMITIVE)
            return set_error(VXG_ERR_NOT_IMPLEMENTED, "filter supports primitive, bool and utf8/binary dtypes");
    }
    vxg_filter_batch_info fi{};
    const std::vector<vxg_canonical> in(outs, outs + n_columns);
    vxg_status st;
    {
        Planner p(ctx, S(stream));
        st = p.filter_batch(columns, n_columns, mask, len, flags, outs, true_count, fi);
    }
    if (info) *info = fi;
    if (st != VXG_OK) {  // nothing engine-allocated is handed back with an error
        (void)hipStreamSynchronize(S(stream));  // (launches of earlier columns may still write them)
        for (uint32_t i = 0; i < n_columns; i++) {
            void* const cur[4] = {outs[i].values, outs[i].validity, outs[i].views, outs[i].data};
            void* const was[4] = {in[i].values, in[i].validity, in[i].views, in[i].data};
            for (int b = 0; b < 4; b++)
                if (cur[b] && cur[b] != was[b]) (void)hipFree(cur[b]);
            outs[i] = in[i];
        }
    }
    return st;
}

vxg_status vxg_runend_bool_decode(vxg_ctx* ctx, int ends_ptype, const void* ends, uint64_t n_runs, uint64_t offset,
                                  int start, uint64_t len, void* out_bits, uint64_t out_bit_offset, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_unsigned(ends_ptype))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "Ends array must be an unsigned integer type");
    if (len && (!out_bits || (n_runs && !ends))) return set_error(VXG_ERR_INVALID_ARGUMENT, "null ends/output");
    return launch_runend_bool(ends, ptype_width(ends_ptype), n_runs, offset, start != 0, len, out_bits,
                              out_bit_offset, ctx->c.err_word, S(stream));
}

vxg_status vxg_bytebool_to_bits(vxg_ctx* ctx, const uint8_t* bytes, uint64_t n, void* out_bits,
                                uint64_t out_bit_offset, void* stream) {
    VXG_TRY(use_device(ctx));
    if (n && (!bytes || !out_bits)) return set_error(VXG_ERR_INVALID_ARGUMENT, "null input/output");
    return launch_bytebool(bytes, n, out_bits, out_bit_offset, S(stream));
}

uint64_t vxg_fsst_scratch_bytes(uint64_t n) { return fsst_scratch_bytes(n); }

vxg_status vxg_fsst_decode(vxg_ctx* ctx, const uint64_t* symbols, const uint8_t* sym_lens, unsigned n_symbols,
                           const uint8_t* code_bytes, int offs_ptype, const void* code_offsets, int lens_ptype,
                           const void* lens, uint64_t n, const uint8_t* validity, void* scratch, uint8_t* heap,
                           uint8_t* views, void* stream) {
    VXG_TRY(use_device(ctx));
    if (!ptype_is_int(offs_ptype) || !ptype_is_int(lens_ptype))
        return set_error(VXG_ERR_MISMATCHED_TYPES, "FSST offsets/lengths must be integers");
    if (n_symbols > 255) return set_error(VXG_ERR_INVALID_ARGUMENT, "FSST symbol table > 255 entries");
    // (code_bytes and heap may be null when every string is empty: no byte of either is touched)
    if ((n_symbols && (!symbols || !sym_lens)) || (n && (!code_offsets || !lens || !scratch || !views)))
        return set_error(VXG_ERR_INVALID_ARGUMENT, "null symbols/offsets/lengths/scratch/views");
    FsstChunk f{};
    f.symbols = symbols;
    f.sym_lens = sym_lens;
    f.n_symbols = n_symbols;
    f.codes = code_bytes;
    f.offs.p = code_offsets;
    f.offs.width = ptype_width(offs_ptype);
    f.offs.sgn = ptype_is_signed(offs_ptype);
    f.lens.p = lens;
    f.lens.width = ptype_width(lens_ptype);
    f.lens.sgn = ptype_is_signed(lens_ptype);
    f.n = n;
    f.validity = validity;
    f.heap = heap;
    f.views = views;
    std::vector<FsstChunk> one{f};
    return launch_fsst_batch(one, scratch, ctx->c.err_word, S(stream));
}

vxg_status vxg_fill(vxg_ctx* ctx, unsigned value_width, const void* scalar_host, uint64_t n, void* out,
                    void* stream) {
    VXG_TRY(use_device(ctx));
    uint8_t sc[16] = {0};
    if (!value_width_ok(value_width)) return set_error(VXG_ERR_INVALID_ARGUMENT, "value width must be 1, 2, 4, 8 or 16");
    if (n == 0) return VXG_OK;
    if (!scalar_host || !out) return set_error(VXG_ERR_INVALID_ARGUMENT, "null scalar/out");
    std::memcpy(sc, scalar_host, value_width);
    return launch_fill(int(value_width), sc, n, out, S(stream));
}

}  // extern "C"
