// Transform::getMaxEncodedLength of the transforms the device runs: the most a forward stage may write for n bytes, which sizes the
// buffers of a chain. One copy for the device driver (api.hip) and the host mirror (host/kanzi_amd.cpp).
#pragma once
#include "knz_hip.h"

inline int knz_max_encoded_len(int t, int n)
{
    switch (t) {
    case KNZ_T_BWT: return n + 33;                                                     // BWTBlockCodec.hpp:47-50
    case KNZ_T_SRT: return n + 1024;                                                   // SRT.hpp:38
    case KNZ_T_PACK: case KNZ_T_DNA: return n + 1024;                                                  // AliasCodec.hpp:52-55
    case KNZ_T_MM: return n + (n < 1024 ? 64 : n >> 4);                                // FSDCodec.hpp:45-48
    case KNZ_T_RLT: return (n <= 512) ? n + 32 : n;                                    // RLT.hpp:43
    case KNZ_T_LZ: case KNZ_T_LZX: return ((n <= 1024) ? n + 16 : n + n / 64) + 2;     // LZCodec.hpp:91-95
    case KNZ_T_LZP: return (n <= 1024) ? n + 16 : n + n / 64;                           // LZCodec.hpp:158-161
    case KNZ_T_ROLZX: return n + (n < 32768 ? 1024 : n >> 5);                          // ROLZCodec.hpp:168-173
    case KNZ_T_EXE: return (n <= 256) ? n + 32 : n + n / 8;                            // EXECodec.hpp:96-100
    case KNZ_T_UTF: return n + 8192;                                                   // UTFCodec.hpp:53
    default: return n;
    }
}
