// Which instantiations of k_solve_wave (cnf_wave.hip) exist: the one statement of it.  A query names a FORM of the kernel and
// what the network looks like -- 16-row tiles of the input and of the hidden layer, the compute mode, whether the second layer's
// activation is tanh or the identity -- and gets the ten template arguments of the instantiation that runs it, or nothing.
// cnf_wave.hip maps those arguments to the kernel (wave_instance) and instantiates nothing else.
//
// The first layer's activation is not part of a query: every activation of the library runs on the plain form, and the callers
// of the other forms (wave_grad_supported, ens_fn, wave_solve_launch) ask for tanh there before they ask here.
//
// Plain C++ (no HIP), like cnf_record.h: tests/support/wave_variants_test.cpp walks the whole query space against the table
// the selection functions before this header answered with (tests/support/wave_variants.expected).
#pragma once
#include <optional>

enum WaveMode { WVM_VJP = 0, WVM_JVP = 1, WVM_TEST = 2 };       // TrainMode by VJP, TrainMode by JVP, TestMode (the exact trace)

enum WaveForm {
    WF_PLAIN = 0,      // one wave per workgroup and tile, the tiles meeting through tagged words (up to 512 of them)
    WF_WG4,            // up to four waves per workgroup meeting through LDS; beyond 512 tiles, workgroups of four
    WF_GRAD,           // the solve, the loss sums and the discrete adjoint: a tile's main wave and its helper
    WF_GRAD_RICH,      // ... whose forward pass files its intermediates (TrainMode / VJP only)
    WF_ENS_GRAD,       // WF_GRAD of M members in one launch (no RICH form: its gradient is the recomputing form's bit for bit,
                       // and the ensemble is there to fill the chip, not to save products)
    WF_ENS_PLAIN,      // M members scored or sampled in one launch: the envelope of WF_ENS_GRAD, so that every ensemble that
                       // can be trained in one launch can be scored and sampled in one
    WF_PATH,           // the solve's state at caller-given times
    WF_COUNT
};

// the template arguments of k_solve_wave, in its order
struct WaveVariant {
    int ni, nh;        // NI, NH: 16-row tiles of the input and of the hidden layer
    int mode;          // MODE
    bool tanh;         // TANH: tanh compiled in as the second layer's activation (false: cnf_act decides at run time)
    bool grad;         // GRAD
    bool id2;          // ID2: the second layer's activation is the identity, compiled out
    int wgw;           // WGW: waves (tiles) per workgroup
    bool rich, ens, path;                                  // RICH, ENS, PATH
};
inline bool operator==(const WaveVariant& a, const WaveVariant& b) {
    return a.ni == b.ni && a.nh == b.nh && a.mode == b.mode && a.tanh == b.tanh && a.grad == b.grad && a.id2 == b.id2 &&
           a.wgw == b.wgw && a.rich == b.rich && a.ens == b.ens && a.path == b.path;
}

// tanh2 / id2: the network's second activation is tanh / it is (tanh, identity) -- a one-layer tanh network with its appended
// identity layer, or a PlanarLayer.  Where both are set the identity wins, as it is the network's.
inline std::optional<WaveVariant> wave_variant(WaveForm form, int ni, int nh, int mode, bool tanh2, bool id2) {
    if (mode != WVM_VJP && mode != WVM_JVP && mode != WVM_TEST) return std::nullopt;
    const bool narrow = ni == 1 && nh >= 1 && nh <= 4;     // n_in <= 16 with up to 64 hidden units
    WaveVariant v{ni, nh, mode, true, false, false, 1, false, false, false};
    switch (form) {
        case WF_PLAIN:                                     // (1, 1..4) or (2, 6): 32 -> 96 -> 32; any second activation
            if (!narrow && !(ni == 2 && nh == 6)) return std::nullopt;
            v.id2 = id2 && nh == 1;                        // (compiled out at one tile each; elsewhere the identity runs as any
            v.tanh = v.id2 || tanh2;                       //  activation that is not tanh)
            return v;
        case WF_WG4:                                       // tanh networks; no JVP on the identity form
            if (!narrow || !(tanh2 || id2) || (id2 && (nh != 1 || mode == WVM_JVP))) return std::nullopt;
            v.id2 = id2; v.wgw = 4;
            return v;
        case WF_GRAD_RICH:
            if (mode != WVM_VJP) return std::nullopt;
            [[fallthrough]];
        case WF_GRAD:
        case WF_ENS_GRAD:
        case WF_ENS_PLAIN:
        case WF_PATH:                                      // tanh networks; the identity second layer only with one hidden tile
            if (!narrow || (id2 && nh != 1) || (form == WF_PATH && !(tanh2 || id2))) return std::nullopt;
            v.id2 = id2;
            v.grad = form != WF_ENS_PLAIN && form != WF_PATH;
            v.rich = form == WF_GRAD_RICH;
            v.ens = form == WF_ENS_GRAD || form == WF_ENS_PLAIN;
            v.path = form == WF_PATH;
            return v;
        default: return std::nullopt;
    }
}
