// Global::DataType and Global::detectSimpleType (Global.cpp:354-), shared by the stages that read and write the per-block data type
// (pack.hip, mm.hip).
#pragma once
#include "common.hpp"

namespace knz {

enum { DT_UNDEFINED = 0, DT_TEXT, DT_MULTIMEDIA, DT_EXE, DT_NUMERIC, DT_BASE64, DT_DNA, DT_BIN, DT_UTF8, DT_SMALL_ALPHABET };

__device__ inline int pk_simple_type(u32 count, const u32* f0)            // Global::detectSimpleType
{
    const char dna[] = "acgntuACGNTU";
    const char num[] = "0123456789+-*/=,.:; ";
    const char b64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    int sum = 0;
    for (int i = 0; i < 12; i++) sum += (int)f0[(u8)dna[i]];
    if (sum > (int)count - (int)count / 12) return DT_DNA;
    sum = 0;
    for (int i = 0; i < 20; i++) sum += (int)f0[(u8)num[i]];
    if (sum == (int)count) return DT_NUMERIC;
    sum = (f0[0x3D] == 1) ? 1 : 0;
    for (int i = 0; i < 64; i++) sum += (int)f0[(u8)b64[i]];
    if (sum == (int)count) return DT_BASE64;
    int distinct = 0;
    for (int i = 0; i < 256; i++) distinct += f0[i] ? 1 : 0;
    if (distinct == 256) return DT_BIN;
    return distinct <= 4 ? DT_SMALL_ALPHABET : DT_UNDEFINED;
}

}  // namespace knz
