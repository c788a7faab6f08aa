// Shared by jpegenc.hip (device half of the JPEG output path) and jpegenc_host.hip (tables, headers, segment gathering).
#pragma once
#include <cstddef>
#include <cstdint>

// Most bits one 8 x 8 block can code to with the Annex-K tables: a DC code of at most 11 bits + 11 value bits, and 63
// times an AC code of at most 16 bits + 10 value bits = 1660 bits, 208 bytes; an MCU of 4:2:0 has six blocks.
constexpr int FM_JPEGENC_BLOCK_BITS = 22 + 63 * 26;
constexpr int FM_JPEGENC_MCU_BYTES = 6 * ((FM_JPEGENC_BLOCK_BITS + 7) / 8);
// Code look-ups for the device, per table set (0: luminance, 1: chrominance): 16 DC entries indexed by the category,
// 256 AC entries indexed by (run << 4) | category; an entry is (code << 5) | code length, 0: no such symbol.
constexpr int FM_JPEGENC_TABLE_WORDS = 16 + 256;

void fm_jpegenc_code_tables(uint32_t* out);          // [2 * FM_JPEGENC_TABLE_WORDS]
// Bytes one MCU row's entropy-coded segment can take BEFORE byte stuffing, as the device buffers space the rows: the
// worst case and the padding byte, rounded up to 16, plus one spare 16-byte unit (a multiple of 16)
size_t fm_jpegenc_row_bytes(int mcus_x);
