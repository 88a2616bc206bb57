// Environment switches of the row-block path (dtqn_tiled.hip, dtqn_wpack.hpp): the one table of their names and the one place that reads them.
// Host only.  Every switch is an A/B or test handle: unset, the rule named in its line decides (DESIGN.md 3.2 has the same table).
// They are read per call and never cached -- tests flip them between two updates of one process -- and once per pass: tl_fwd_plan /
// tl_bwd_plan (dtqn_tiled.hip) turn them into the decisions the launchers are handed.
#pragma once
#include <cstdlib>

namespace dtqn {

// How a switch is parsed.  The kinds are historical and kept as they are: scripts and tests set the variables in these forms.
enum TlSwKind {
    TL_SW_SET,                         // set at all, whatever the text ("=0" counts as set)
    TL_SW_ONE,                         // first character '1'
    TL_SW_INT,                         // atoi of the text; unset: the rule decides
};

// X(id, "NAME", kind, "meaning; what decides when it is unset")
#define DTQN_TL_SWITCHES(X)                                                                                                                  \
    X(TL_TRACE, "DTQN_TL_TRACE", TL_SW_ONE, "one line per launch on stderr (read per launch); off")                                           \
    X(NO_WIDE, "DTQN_NO_WIDE", TL_SW_SET, "no column-walking kernels (tl_wide, and with it the fused layer tail and the fused projections); they run")   \
    X(ATTN_KBLOCK, "DTQN_ATTN_KBLOCK", TL_SW_ONE, "key-blocked attention on any shape; only where one head's tile does not fit LDS")           \
    X(BAG_ATTN_MFMA, "DTQN_BAG_ATTN_MFMA", TL_SW_ONE, "matrix-core bag attention on any bag; only where the resident backward does not fit LDS") \
    X(LAYER_FUSE, "DTQN_LAYER_FUSE", TL_SW_INT, "0: separate launches behind the attention; post-LN residual layers run tl_layer_kernel")      \
    X(QKV_FUSE, "DTQN_QKV_FUSE", TL_SW_INT, "0: the next layer's q|k|v projection in its own launch; it rides in the layer launch (64 rows, d_model 128 / 256)") \
    X(EMBED_QKV, "DTQN_EMBED_QKV", TL_SW_INT, "0 | 1: layer 0's q|k|v projection apart from / inside the table embedding; inside at d_model 128 from two rounds on") \
    X(PACK_ROWS, "DTQN_PACK_ROWS", TL_SW_INT, "0: every workgroup on (sequence, row block); the unsaved passes walk their live rows (TlPack)") \
    X(HEAD_FUSE, "DTQN_HEAD_FUSE", TL_SW_INT, "0: tl_head_bwd_kernel in its own launch; the Q-head backward rides in the dL/dxf product (no bag)") \
    X(BWD_CHAIN, "DTQN_BWD_CHAIN", TL_SW_INT, "0: separate backward launches; post-LN residual layers run tl_chain_bwd_kernel")               \
    X(BWD_CHAIN256, "DTQN_BWD_CHAIN256", TL_SW_INT, "0 | 1: the chain kernel at d_model 256; only beside a side stream")                       \
    X(FFN_BWD, "DTQN_FFN_BWD", TL_SW_INT, "0 | 1: separate products / fused feed-forward backward; fused at d_model <= 128")                   \
    X(FFN_ROWS, "DTQN_FFN_ROWS", TL_SW_INT, "32 | 64 rows per workgroup of the feed-forward, wide and layer kernels; by launch size")          \
    X(ROWS_FFN, "DTQN_ROWS_FFN", TL_SW_INT, "the same for tl_ffn / tl_layer alone; DTQN_FFN_ROWS")                                             \
    X(ROWS_FFNB, "DTQN_ROWS_FFNB", TL_SW_INT, "the same for tl_ffn_bwd / tl_chain_bwd alone; DTQN_FFN_ROWS")                                   \
    X(ROWS_WIDE, "DTQN_ROWS_WIDE", TL_SW_INT, "the same for tl_wide alone; DTQN_FFN_ROWS")                                                     \
    X(GEMM_ROWS, "DTQN_GEMM_ROWS", TL_SW_INT, "32 | auto: 32-row tl_linear / tl_dx workgroups always / for launches that idle 40 % of their slots; 64 rows") \
    X(SKEW_TICKS, "DTQN_SKEW_TICKS", TL_SW_INT, "start skew of a round-and-a-half launch in 100-MHz ticks; 600 (layer kernel 2000)")           \
    X(SKEW_WIDE, "DTQN_SKEW_WIDE", TL_SW_INT, "the same for tl_wide alone; DTQN_SKEW_TICKS")                                                   \
    X(SKEW_LAYER, "DTQN_SKEW_LAYER", TL_SW_INT, "the same for tl_layer alone; DTQN_SKEW_TICKS")                                                \
    X(WPACK, "DTQN_WPACK", TL_SW_INT, "0: the kernels read the parameter layout; fragment-major weight copies at d_model 128 / 256")           \
    X(EMBED_TABLE, "DTQN_EMBED_TABLE", TL_SW_INT, "0: discrete observations through the matrix product; through the product table")

enum TlSw {
#define DTQN_TL_SW_ID(id, name, kind, meaning) TLSW_##id,
    DTQN_TL_SWITCHES(DTQN_TL_SW_ID)
#undef DTQN_TL_SW_ID
    TLSW_COUNT
};
struct TlSwInfo {
    const char* name;
    TlSwKind kind;
    const char* meaning;
};
constexpr TlSwInfo kTlSwitches[TLSW_COUNT] = {
#define DTQN_TL_SW_ROW(id, name, kind, meaning) {name, kind, meaning},
    DTQN_TL_SWITCHES(DTQN_TL_SW_ROW)
#undef DTQN_TL_SW_ROW
};

// One reader per kind; the template argument ties every read to the table (a switch read with the wrong kind's reader does not compile).
template <TlSw S>
static inline bool tl_sw_set() {
    static_assert(kTlSwitches[S].kind == TL_SW_SET, "not a presence switch");
    return getenv(kTlSwitches[S].name) != nullptr;
}
template <TlSw S>
static inline bool tl_sw_one() {
    static_assert(kTlSwitches[S].kind == TL_SW_ONE, "not a first-character switch");
    const char* e = getenv(kTlSwitches[S].name);
    return e != nullptr && e[0] == '1';
}
struct TlSwInt {
    bool set;
    int v;                             // atoi of the text (0 when unset)
    char c0;                           // first character of the text (DTQN_GEMM_ROWS=auto)
    bool on(bool rule) const { return set ? v != 0 : rule; }
    int or_else(int rule) const { return set ? v : rule; }
};
// S, or where S is unset the family switch FB (DTQN_ROWS_* -> DTQN_FFN_ROWS, DTQN_SKEW_WIDE / _LAYER -> DTQN_SKEW_TICKS)
template <TlSw S, TlSw FB = S>
static inline TlSwInt tl_sw_int() {
    static_assert(kTlSwitches[S].kind == TL_SW_INT && kTlSwitches[FB].kind == TL_SW_INT, "not an integer switch");
    const char* e = getenv(kTlSwitches[S].name);
    if (e == nullptr && FB != S) e = getenv(kTlSwitches[FB].name);
    return e != nullptr ? TlSwInt{true, atoi(e), e[0]} : TlSwInt{false, 0, '\0'};
}

}  // namespace dtqn
