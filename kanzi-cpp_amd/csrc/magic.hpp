// Magic numbers of a block's first 4 bytes and the data type the reference presets from them (Magic.hpp:64-170,
// io/CompressedOutputStream.cpp:722-731). One copy for the host stages (host/text_codec.cpp) and the device chains (sequence.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KNZ_HD __host__ __device__
#else
#define KNZ_HD
#endif

namespace knz_magic {

enum { DT_UNDEFINED = 0, DT_MULTIMEDIA = 2, DT_EXE = 3, DT_BIN = 7 };

// Magic::getType: the recognised magic, 0 (NO_MAGIC) otherwise
KNZ_HD inline uint32_t magic_of(const uint8_t* p)
{
    const uint32_t k = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
    if ((k & ~0x0Fu) == 0xFFD8FFE0u) return k;                                  // JPEG (the low nibble stays in the value)
    if ((k >> 8) == 0x425A68u || (k >> 8) == 0x494433u) return k >> 8;          // bzip2, ID3
    switch (k) {
    case 0x47494638u /* GIF */: case 0x25504446u /* PDF */: case 0x504B0304u /* ZIP */: case 0x377ABCAFu /* 7z */: case 0x89504E47u /* PNG */:
    case 0x7F454C46u /* ELF */: case 0xFEEDFACEu: case 0xCEFAEDFEu: case 0xFEEDFACFu: case 0xCFFAEDFEu /* Mach-O */: case 0x28B52FFDu /* zstd */:
    case 0x81CFB2CEu /* brotli */: case 0x4D534346u /* CAB */: case 0x52494646u /* RIFF */: case 0x664C6143u /* FLAC */: case 0xFD377A58u /* xz */:
    case 0x4B414E5Au /* KANZ */: case 0x52617221u /* RAR */:
        return k;
    default: break;
    }
    const uint32_t k16 = k >> 16;
    if (k16 == 0x1F8Bu || k16 == 0x424Du || k16 == 0x4D5Au) return k16;         // gzip, BMP, MZ
    if (k16 == 0x5034u || k16 == 0x5035u || k16 == 0x5036u) {                   // binary PBM / PGM / PPM: "P4".."P6" + white space
        const uint32_t c = (k >> 8) & 0xFF;
        if (c == 0x07 || c == 0x0A || c == 0x0D || c == 0x20) return k16;
    }
    return 0;
}

KNZ_HD inline bool magic_compressed(uint32_t m)
{
    switch (m) {
    case 0xFFD8FFE0u: case 0x47494638u: case 0x89504E47u: case 0x377ABCAFu: case 0x28B52FFDu: case 0x81CFB2CEu: case 0x4D534346u: case 0x504B0304u:
    case 0x1F8Bu: case 0x425A68u: case 0x664C6143u: case 0x494433u: case 0xFD377A58u: case 0x4B414E5Au: case 0x52617221u:
        return true;
    default:
        return false;
    }
}

KNZ_HD inline bool magic_multimedia(uint32_t m)
{
    switch (m) {
    case 0xFFD8FFE0u: case 0x47494638u: case 0x89504E47u: case 0x52494646u: case 0x664C6143u: case 0x494433u: case 0x424Du: case 0x5034u: case 0x5035u: case 0x5036u:
        return true;
    default:
        return false;
    }
}

KNZ_HD inline bool magic_executable(uint32_t m)
{
    switch (m) {
    case 0x7F454C46u: case 0x4D5Au: case 0xFEEDFACEu: case 0xCEFAEDFEu: case 0xFEEDFACFu: case 0xCFFAEDFEu:
        return true;
    default:
        return false;
    }
}

// the "dataType" a block starts with: BIN, MULTIMEDIA, EXE or UNDEFINED (checked in that order)
KNZ_HD inline int data_type_preset(const uint8_t* block, uint32_t n)
{
    if (n < 4) return DT_UNDEFINED;
    const uint32_t m = magic_of(block);
    if (magic_compressed(m)) return DT_BIN;
    if (magic_multimedia(m)) return DT_MULTIMEDIA;
    if (magic_executable(m)) return DT_EXE;
    return DT_UNDEFINED;
}

}  // namespace knz_magic
