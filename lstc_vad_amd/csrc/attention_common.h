// Shared by the attention translation units (csrc/attention.hip: first / second generation kernels, CLS kernels, the C-ABI entry
// points; csrc/attention_pk.hip: the packed-operand kernels of the bf16 mode; csrc/attention_long.hip: the key-tiled kernels for
// 128 < S <= 512).
#pragma once
#include "lstc_common.h"
#include <type_traits>

namespace lstc_attn {

struct AttnParams {
    const float *Q, *K, *V;
    float* O;
    float* probs;
    const float* table;
    const int64_t* index;
    const float* dO;
    float *dQ, *dK, *dV;
    float* dtable;
    int N, S, H, dk, dv, ldq, ldk, ldv, ldo, index_ld, table_rows;
    float scale;
    DropKey dkey;
    int has_drop;
    int vec_qk, vec_v;     // float4 operand loads allowed for the dk / dv contractions
    int n_per_wg;
    int table_partials;     // 1: dtable is [gridDim.x][table_rows][H] partials (plain stores), 0: [rows][H] with atomics
    // bf16 mode (staged backward only): dQ / dK / dV written as packed bf16 operands [N*S, H*dk|dv] (lstc_pack1 layout) instead
    // of f32 - they are consumed only by the packed weight-gradient and input-gradient GEMMs
    void *dQp, *dKp, *dVp;
    int kbq, kbk, kbv;      // 32-k tiles per 128-row block of each pack
    int tq0, tk0, tv0;      // first k tile of the dQ / dK / dV columns inside their pack (one fused pack: column offsets / 32)
    void* Op;               // forward, bf16 mode: O written as a packed bf16 operand [N*S, H*dv] instead of f32
    int kbo;
    // bf16 mode, packed INPUTS (third-generation kernels): Q / K / V / dO are lstc_pack1 buffers; 32-k tiles per 128-row block of
    // each pack and the first tile of head 0's columns inside it
    const __bf16 *Qi, *Ki, *Vi, *dOi;
    int kiq, kik, kiv, kido;
    int iq0, ik0, iv0, ido0;
    int pld;                // row pitch of `probs` in floats (packed-input kernels: a multiple of 4, >= S; else S)
};

// Attention mask of the *_masked entry points (LstcAttnMask): one byte per (n, h, query i, key j) through four element strides
// (0 = broadcast); byte 0 = masked.  The second argument of every maskable kernel is a MaskArg<MASKED>: the mask for the masked
// instantiation, an empty NoMask for the unmasked one, whose body then holds no trace of it (`if constexpr (MASKED)`).
struct MaskParams {
    const uint8_t* m;
    int64_t sn, sh, sq, sk;
};
struct NoMask {};
template <bool MASKED>
using MaskArg = std::conditional_t<MASKED, MaskParams, NoMask>;
// the logit of a masked position, in place of the scaled q.k and before the relative bias (the reference's masked_fill value);
// -1e9f + bias rounds back to -1e9f for |bias| < 32, so a fully masked row comes out uniform and nothing is ever -inf or NaN
constexpr float ATTN_MASK_FILL = -1e9f;

// Sequence offsets of the *_var entry points (LstcSeqs): the tokens of all sequences lie back to back in [M, ld] matrices, sequence
// n = rows row0[n] .. row0[n + 1] - 1, its probabilities H * S_n * S_n floats from prob0[n]; a launch covers the n_ids sequences
// ids[0 .. n_ids) (ids null: 0 .. n_ids - 1).  The third argument of the first-generation kernel bodies (S_n <= 128) and of the
// key-tiled ones (csrc/attention_long.hip, S_n <= 512) is a SeqArg<VAR>, empty for the fixed-S kernels, whose code then holds no
// trace of it (`if constexpr (VAR)`, or the overloads below that fold to the fixed-S value).
struct SeqParams {
    const int32_t* row0;
    const int64_t* prob0;
    const int32_t* ids;
    int n_ids;
};
struct NoSeqs {};
template <bool VAR>
using SeqArg = std::conditional_t<VAR, SeqParams, NoSeqs>;
// sequences of the launch, spelled so that the fixed-S instantiation compiles too (it never reads the value)
__device__ __forceinline__ int seq_count(const SeqParams& sq) { return sq.n_ids; }
__device__ __forceinline__ int seq_count(const NoSeqs&) { return 0; }
// sequence of position `it` of the launch, its length clamped to [1, cap] and its first row
__device__ __forceinline__ int seq_id(const SeqParams& sq, int it) { return sq.ids ? sq.ids[it] : it; }
__device__ __forceinline__ int seq_id(const NoSeqs&, int it) { return it; }
__device__ __forceinline__ int seq_len(const SeqParams& sq, int n, int cap) { return min(max(sq.row0[n + 1] - sq.row0[n], 1), cap); }
__device__ __forceinline__ int seq_len(const NoSeqs&, int, int) { return 0; }
__device__ __forceinline__ size_t seq_row0(const SeqParams& sq, int n) { return (size_t)sq.row0[n]; }
__device__ __forceinline__ size_t seq_row0(const NoSeqs&, int) { return 0; }

typedef __bf16 attn_h8 __attribute__((ext_vector_type(8)));
typedef float attn_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 attn_h2 __attribute__((ext_vector_type(2)));

// csrc/attention_pk.hip: launch the packed-operand kernels (LstcAttnDesc.in_pack_cols > 0) for T = ceil(S / 32) in 1..3 over
// `chunks` groups of p.n_per_wg sequences x p.H heads; 0 or LSTC_E_* / hipError_t as the entry points return it
// (internal to the library: not part of the C ABI, hidden from the dynamic symbol table)
__attribute__((visibility("hidden"))) int attn3_fwd_launch(const AttnParams& p, int T, int chunks, hipStream_t st);
__attribute__((visibility("hidden"))) int attn3_bwd_launch(const AttnParams& p, int T, int chunks, hipStream_t st);
// exact-f32 forward on the same structure (f32 operands, dense probs): csrc/attention_pk.hip
__attribute__((visibility("hidden"))) int attn3f_fwd_launch(const AttnParams& p, int T, int chunks, hipStream_t st);
// csrc/attention_long.hip: the key-tiled kernels for 128 < S <= 512 (row inputs and outputs only), called by the forward /
// backward entry points after fill_params; check their own preconditions, then launch.  mk: the attention mask of the *_masked
// entry points (the masked instantiations of the same kernels), null for none
__attribute__((visibility("hidden"))) int attn_long_fwd_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams* mk, hipStream_t st);
__attribute__((visibility("hidden"))) int attn_long_bwd_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams* mk, hipStream_t st);
// the same kernels over sequence offsets (their VAR instantiations, exact-f32 products, no mask), behind lstc_attn_var_long_fwd / _bwd
__attribute__((visibility("hidden"))) int attn_long_var_fwd_launch(const LstcAttnDesc* d, AttnParams& p, const SeqParams& sq, hipStream_t st);
__attribute__((visibility("hidden"))) int attn_long_var_bwd_launch(const LstcAttnDesc* d, AttnParams& p, const SeqParams& sq, hipStream_t st);

// Host side: launch a kernel that asks for more than 64 KB of dynamic LDS.  The opt-in (MAX_LDS bytes; 160 KB = the whole LDS of a
// CU) is a per-device attribute of the kernel: set once per device and kernel instantiation, ahead of its first launch there.
template <auto Kern, int MAX_LDS = 160 * 1024, typename... Args>
void launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
    static LstcDevOnce once;
    const int dev = once.begin();
    if (dev >= 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS);
        once.end(dev);
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
}

}  // namespace lstc_attn
