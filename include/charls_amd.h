/*
 * charls_amd.h -- C ABI of the MI355X-native JPEG-LS engine.
 *
 * Part 1 is the drop-in boundary: the 48 entry points, enums and four POD structs of team-charls/charls 3.0, with the
 * same names, argument meaning, state machines and error codes, so that a program built against the reference's own
 * <charls/charls.h> runs unchanged when libcharls_amd.so is loaded in place of libcharls.so.3.  Each declaration cites
 * the reference interface it replaces (paths relative to the reference tree).  Source/destination buffers passed to
 * part 1 are HOST memory, borrowed for the duration of the call exactly as in the reference.
 *
 * Part 2 (prefix charls_amd_) is additive: batch entry points working on DEVICE-resident frames, which is how the
 * engine is meant to be fed at scale (independent frames / scans are the sharding unit across wavefronts and GPUs).
 *
 * Plain C: opaque handles, plain pointers and sizes, no C++ or torch types cross this boundary
 * (the one exception, charls_get_jpegls_category, is inherited from the reference and documented there).
 */
#ifndef CHARLS_AMD_H
#define CHARLS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define CHARLS_AMD_API __attribute__((visibility("default")))
#else
#define CHARLS_AMD_API
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * Types: include/charls/public_types.h:28-187 (enums), :934-1034 (structs; sizes 40/16/20/12 asserted at :1075-1078)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef int32_t charls_jpegls_errc; /* enum charls_jpegls_errc, int32-sized; values below */
enum
{
    CHARLS_JPEGLS_ERRC_SUCCESS = 0,
    CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY = 1,
    CHARLS_JPEGLS_ERRC_CALLBACK_FAILED = 2,
    CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL = 3,
    CHARLS_JPEGLS_ERRC_NEED_MORE_DATA = 4,
    CHARLS_JPEGLS_ERRC_INVALID_DATA = 5,
    CHARLS_JPEGLS_ERRC_ENCODING_NOT_SUPPORTED = 6,
    CHARLS_JPEGLS_ERRC_PARAMETER_VALUE_NOT_SUPPORTED = 7,
    CHARLS_JPEGLS_ERRC_COLOR_TRANSFORM_NOT_SUPPORTED = 8,
    CHARLS_JPEGLS_ERRC_JPEGLS_PRESET_EXTENDED_PARAMETER_TYPE_NOT_SUPPORTED = 9,
    CHARLS_JPEGLS_ERRC_JPEG_MARKER_START_BYTE_NOT_FOUND = 10,
    CHARLS_JPEGLS_ERRC_START_OF_IMAGE_MARKER_NOT_FOUND = 11,
    CHARLS_JPEGLS_ERRC_INVALID_SPIFF_HEADER = 12,
    CHARLS_JPEGLS_ERRC_UNKNOWN_JPEG_MARKER_FOUND = 13,
    CHARLS_JPEGLS_ERRC_UNEXPECTED_START_OF_SCAN_MARKER = 14,
    CHARLS_JPEGLS_ERRC_INVALID_MARKER_SEGMENT_SIZE = 15,
    CHARLS_JPEGLS_ERRC_DUPLICATE_START_OF_IMAGE_MARKER = 16,
    CHARLS_JPEGLS_ERRC_DUPLICATE_START_OF_FRAME_MARKER = 17,
    CHARLS_JPEGLS_ERRC_DUPLICATE_COMPONENT_ID_IN_SOF_SEGMENT = 18,
    CHARLS_JPEGLS_ERRC_UNEXPECTED_END_OF_IMAGE_MARKER = 19,
    CHARLS_JPEGLS_ERRC_INVALID_JPEGLS_PRESET_PARAMETER_TYPE = 20,
    CHARLS_JPEGLS_ERRC_MISSING_END_OF_SPIFF_DIRECTORY = 21,
    CHARLS_JPEGLS_ERRC_UNEXPECTED_RESTART_MARKER = 22,
    CHARLS_JPEGLS_ERRC_RESTART_MARKER_NOT_FOUND = 23,
    CHARLS_JPEGLS_ERRC_END_OF_IMAGE_MARKER_NOT_FOUND = 24,
    CHARLS_JPEGLS_ERRC_UNEXPECTED_DEFINE_NUMBER_OF_LINES_MARKER = 25,
    CHARLS_JPEGLS_ERRC_DEFINE_NUMBER_OF_LINES_MARKER_NOT_FOUND = 26,
    CHARLS_JPEGLS_ERRC_UNKNOWN_COMPONENT_ID = 27,
    CHARLS_JPEGLS_ERRC_ABBREVIATED_FORMAT_AND_SPIFF_HEADER_MISMATCH = 28,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_WIDTH = 29,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_HEIGHT = 30,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_BITS_PER_SAMPLE = 31,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_COMPONENT_COUNT = 32,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_INTERLEAVE_MODE = 33,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_NEAR_LOSSLESS = 34,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_JPEGLS_PRESET_PARAMETERS = 35,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_COLOR_TRANSFORMATION = 36,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_MAPPING_TABLE_ID = 37,
    CHARLS_JPEGLS_ERRC_INVALID_PARAMETER_MAPPING_TABLE_CONTINUATION = 38,
    CHARLS_JPEGLS_ERRC_INVALID_OPERATION = 100,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT = 101,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_WIDTH = 102,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_HEIGHT = 103,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_BITS_PER_SAMPLE = 104,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COMPONENT_COUNT = 105,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_INTERLEAVE_MODE = 106,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_NEAR_LOSSLESS = 107,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_JPEGLS_PC_PARAMETERS = 108,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COLOR_TRANSFORMATION = 109,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE = 110,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE = 111,
    CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_ENCODING_OPTIONS = 112,
    /* additive, never produced by the reference: the engine has no CPU fallback, so a missing / failing GPU is an error */
    CHARLS_AMD_ERRC_DEVICE_UNAVAILABLE = 200,
    CHARLS_AMD_ERRC_DEVICE_FAILURE = 201
};

/* The reference declares these as C enums (include/charls/public_types.h:90-187); an enum of these values is an int,
 * so 32-bit integer types with the same constant names give a C caller the same source and the same ABI. */
typedef int32_t charls_interleave_mode;
enum { CHARLS_INTERLEAVE_MODE_NONE = 0, CHARLS_INTERLEAVE_MODE_LINE = 1, CHARLS_INTERLEAVE_MODE_SAMPLE = 2 };
typedef int32_t charls_color_transformation;
enum { CHARLS_COLOR_TRANSFORMATION_NONE = 0, CHARLS_COLOR_TRANSFORMATION_HP1 = 1, CHARLS_COLOR_TRANSFORMATION_HP2 = 2,
       CHARLS_COLOR_TRANSFORMATION_HP3 = 3 };
typedef uint32_t charls_encoding_options;
enum { CHARLS_ENCODING_OPTIONS_NONE = 0, CHARLS_ENCODING_OPTIONS_EVEN_DESTINATION_SIZE = 1,
       CHARLS_ENCODING_OPTIONS_INCLUDE_VERSION_NUMBER = 2, CHARLS_ENCODING_OPTIONS_INCLUDE_PC_PARAMETERS_JAI = 4 };
typedef int32_t charls_compressed_data_format;
enum { CHARLS_COMPRESSED_DATA_FORMAT_UNKNOWN = 0, CHARLS_COMPRESSED_DATA_FORMAT_INTERCHANGE = 1,
       CHARLS_COMPRESSED_DATA_FORMAT_ABBREVIATED_IMAGE_DATA = 2, CHARLS_COMPRESSED_DATA_FORMAT_ABBREVIATED_TABLE_SPECIFICATION = 3 };
typedef int32_t charls_spiff_profile_id;
enum { CHARLS_SPIFF_PROFILE_ID_NONE = 0, CHARLS_SPIFF_PROFILE_ID_CONTINUOUS_TONE_BASE = 1,
       CHARLS_SPIFF_PROFILE_ID_CONTINUOUS_TONE_PROGRESSIVE = 2, CHARLS_SPIFF_PROFILE_ID_BI_LEVEL_FACSIMILE = 3,
       CHARLS_SPIFF_PROFILE_ID_CONTINUOUS_TONE_FACSIMILE = 4 };
typedef int32_t charls_spiff_color_space;
enum { CHARLS_SPIFF_COLOR_SPACE_BI_LEVEL_BLACK = 0, CHARLS_SPIFF_COLOR_SPACE_YCBCR_ITU_BT_709_VIDEO = 1,
       CHARLS_SPIFF_COLOR_SPACE_NONE = 2, CHARLS_SPIFF_COLOR_SPACE_YCBCR_ITU_BT_601_1_RGB = 3,
       CHARLS_SPIFF_COLOR_SPACE_YCBCR_ITU_BT_601_1_VIDEO = 4, CHARLS_SPIFF_COLOR_SPACE_GRAYSCALE = 8,
       CHARLS_SPIFF_COLOR_SPACE_PHOTO_YCC = 9, CHARLS_SPIFF_COLOR_SPACE_RGB = 10, CHARLS_SPIFF_COLOR_SPACE_CMY = 11,
       CHARLS_SPIFF_COLOR_SPACE_CMYK = 12, CHARLS_SPIFF_COLOR_SPACE_YCCK = 13, CHARLS_SPIFF_COLOR_SPACE_CIE_LAB = 14,
       CHARLS_SPIFF_COLOR_SPACE_BI_LEVEL_WHITE = 15 };
typedef int32_t charls_spiff_compression_type;
enum { CHARLS_SPIFF_COMPRESSION_TYPE_UNCOMPRESSED = 0, CHARLS_SPIFF_COMPRESSION_TYPE_MODIFIED_HUFFMAN = 1,
       CHARLS_SPIFF_COMPRESSION_TYPE_MODIFIED_READ = 2, CHARLS_SPIFF_COMPRESSION_TYPE_MODIFIED_MODIFIED_READ = 3,
       CHARLS_SPIFF_COMPRESSION_TYPE_JBIG = 4, CHARLS_SPIFF_COMPRESSION_TYPE_JPEG = 5, CHARLS_SPIFF_COMPRESSION_TYPE_JPEG_LS = 6 };
typedef int32_t charls_spiff_resolution_units;
enum { CHARLS_SPIFF_RESOLUTION_UNITS_ASPECT_RATIO = 0, CHARLS_SPIFF_RESOLUTION_UNITS_DOTS_PER_INCH = 1,
       CHARLS_SPIFF_RESOLUTION_UNITS_DOTS_PER_CENTIMETER = 2 };
enum { CHARLS_SPIFF_ENTRY_TAG_TRANSFER_CHARACTERISTICS = 2, CHARLS_SPIFF_ENTRY_TAG_COMPONENT_REGISTRATION = 3,
       CHARLS_SPIFF_ENTRY_TAG_IMAGE_ORIENTATION = 4, CHARLS_SPIFF_ENTRY_TAG_THUMBNAIL = 5, CHARLS_SPIFF_ENTRY_TAG_IMAGE_TITLE = 6,
       CHARLS_SPIFF_ENTRY_TAG_IMAGE_DESCRIPTION = 7, CHARLS_SPIFF_ENTRY_TAG_TIME_STAMP = 8,
       CHARLS_SPIFF_ENTRY_TAG_VERSION_IDENTIFIER = 9, CHARLS_SPIFF_ENTRY_TAG_CREATOR_IDENTIFICATION = 10,
       CHARLS_SPIFF_ENTRY_TAG_PROTECTION_INDICATOR = 11, CHARLS_SPIFF_ENTRY_TAG_COPYRIGHT_INFORMATION = 12,
       CHARLS_SPIFF_ENTRY_TAG_CONTACT_INFORMATION = 13, CHARLS_SPIFF_ENTRY_TAG_TILE_INDEX = 14,
       CHARLS_SPIFF_ENTRY_TAG_SCAN_INDEX = 15, CHARLS_SPIFF_ENTRY_TAG_SET_REFERENCE = 16 };
enum { CHARLS_MAPPING_TABLE_MISSING = -1 };

typedef struct charls_spiff_header
{
    charls_spiff_profile_id profile_id;
    int32_t component_count;
    uint32_t height;
    uint32_t width;
    charls_spiff_color_space color_space;
    int32_t bits_per_sample;
    charls_spiff_compression_type compression_type;
    charls_spiff_resolution_units resolution_units;
    uint32_t vertical_resolution;
    uint32_t horizontal_resolution;
} charls_spiff_header;

typedef struct charls_frame_info
{
    uint32_t width;
    uint32_t height;
    int32_t bits_per_sample;
    int32_t component_count;
} charls_frame_info;

typedef struct charls_jpegls_pc_parameters
{
    int32_t maximum_sample_value;
    int32_t threshold1;
    int32_t threshold2;
    int32_t threshold3;
    int32_t reset_value;
} charls_jpegls_pc_parameters;

typedef struct charls_mapping_table_info
{
    int32_t table_id;
    int32_t entry_size;
    uint32_t data_size;
} charls_mapping_table_info;

typedef int32_t (*charls_at_comment_handler)(const void* data, size_t size, void* user_context);
typedef int32_t (*charls_at_application_data_handler)(int32_t application_data_id, const void* data, size_t size,
                                                      void* user_context);

typedef struct charls_jpegls_encoder charls_jpegls_encoder;
typedef struct charls_jpegls_decoder charls_jpegls_decoder;

/* ------------------------------------------------------------------------------------------------------------------
 * Part 1a -- encoder: include/charls/charls_jpegls_encoder.h:25-318, implemented by src/charls_jpegls_encoder.cpp
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_encoder* charls_jpegls_encoder_create(void);                                   /* :25 */
CHARLS_AMD_API void charls_jpegls_encoder_destroy(const charls_jpegls_encoder* encoder);                    /* :33 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_frame_info(charls_jpegls_encoder* encoder,
                                                                       const charls_frame_info* frame_info); /* :42 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_near_lossless(charls_jpegls_encoder* encoder,
                                                                          int32_t near_lossless);            /* :52 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_encoding_options(charls_jpegls_encoder* encoder,
                                                                             charls_encoding_options options); /* :61 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_interleave_mode(charls_jpegls_encoder* encoder,
                                                                            charls_interleave_mode mode);    /* :72 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_preset_coding_parameters(
    charls_jpegls_encoder* encoder, const charls_jpegls_pc_parameters* preset_coding_parameters);           /* :85 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_color_transformation(
    charls_jpegls_encoder* encoder, charls_color_transformation color_transformation);                      /* :99 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_mapping_table_id(charls_jpegls_encoder* encoder,
                                                                             int32_t component_index,
                                                                             int32_t table_id);             /* :110 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_get_estimated_destination_size(
    const charls_jpegls_encoder* encoder, size_t* size_in_bytes);                                           /* :123 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_set_destination_buffer(charls_jpegls_encoder* encoder,
                                                                               void* destination_buffer,
                                                                               size_t destination_size_bytes); /* :136 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_standard_spiff_header(
    charls_jpegls_encoder* encoder, charls_spiff_color_space color_space, charls_spiff_resolution_units resolution_units,
    uint32_t vertical_resolution, uint32_t horizontal_resolution);                                          /* :152 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_spiff_header(charls_jpegls_encoder* encoder,
                                                                           const charls_spiff_header* spiff_header); /* :166 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_spiff_entry(charls_jpegls_encoder* encoder,
                                                                          uint32_t entry_tag, const void* entry_data,
                                                                          size_t entry_data_size_bytes);    /* :182 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_spiff_end_of_directory_entry(
    charls_jpegls_encoder* encoder);                                                                        /* :197 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_comment(charls_jpegls_encoder* encoder,
                                                                      const void* comment, size_t comment_size_bytes); /* :211 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_application_data(charls_jpegls_encoder* encoder,
                                                                               int32_t application_data_id,
                                                                               const void* application_data,
                                                                               size_t application_data_size_bytes); /* :228 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_write_mapping_table(charls_jpegls_encoder* encoder,
                                                                            int32_t table_id, int32_t entry_size,
                                                                            const void* table_data,
                                                                            size_t table_data_size_bytes);  /* :247 */
/* HOT PATH: :264-268 -> charls_jpegls_encoder::encode -> make_scan_codec<scan_encoder>()->encode_scan (src/...encoder.cpp:182-296) */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_encode_from_buffer(charls_jpegls_encoder* encoder,
                                                                           const void* source_buffer,
                                                                           size_t source_size_bytes, uint32_t stride);
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_encode_components_from_buffer(
    charls_jpegls_encoder* encoder, const void* source_buffer, size_t source_size_bytes, int32_t source_component_count,
    uint32_t stride);                                                                                       /* :284 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_create_abbreviated_format(charls_jpegls_encoder* encoder); /* :297 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_get_bytes_written(const charls_jpegls_encoder* encoder,
                                                                          size_t* bytes_written);           /* :306 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_encoder_rewind(charls_jpegls_encoder* encoder);             /* :316 */

/* ------------------------------------------------------------------------------------------------------------------
 * Part 1b -- decoder: include/charls/charls_jpegls_decoder.h:25-295, implemented by src/charls_jpegls_decoder.cpp
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_decoder* charls_jpegls_decoder_create(void);                                   /* :25 */
CHARLS_AMD_API void charls_jpegls_decoder_destroy(const charls_jpegls_decoder* decoder);                    /* :33 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_set_source_buffer(charls_jpegls_decoder* decoder,
                                                                          const void* source_buffer,
                                                                          size_t source_size_bytes);        /* :45 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_read_spiff_header(charls_jpegls_decoder* decoder,
                                                                          charls_spiff_header* spiff_header,
                                                                          int32_t* header_found);           /* :59 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_read_header(charls_jpegls_decoder* decoder);        /* :69 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_get_frame_info(const charls_jpegls_decoder* decoder,
                                                                       charls_frame_info* frame_info);      /* :81 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_get_near_lossless(const charls_jpegls_decoder* decoder,
                                                                          int32_t component_index,
                                                                          int32_t* near_lossless);          /* :95 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_get_interleave_mode(const charls_jpegls_decoder* decoder,
                                                                            int32_t component_index,
                                                                            charls_interleave_mode* interleave_mode); /* :109 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_get_preset_coding_parameters(
    const charls_jpegls_decoder* decoder, int32_t reserved, charls_jpegls_pc_parameters* preset_coding_parameters); /* :123 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_get_color_transformation(
    const charls_jpegls_decoder* decoder, charls_color_transformation* color_transformation);               /* :137 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_get_destination_size(const charls_jpegls_decoder* decoder,
                                                                             uint32_t stride,
                                                                             size_t* destination_size_bytes); /* :151 */
/* HOT PATH: :170-174 -> charls_jpegls_decoder::decode -> make_scan_codec<scan_decoder>()->decode_scan (src/...decoder.cpp:177-201) */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_decode_to_buffer(charls_jpegls_decoder* decoder,
                                                                         void* destination_buffer,
                                                                         size_t destination_size_bytes, uint32_t stride);
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_at_comment(charls_jpegls_decoder* decoder,
                                                                   charls_at_comment_handler handler,
                                                                   void* user_context);                     /* :186 */
CHARLS_AMD_API charls_jpegls_errc charls_jpegls_decoder_at_application_data(
    charls_jpegls_decoder* decoder, charls_at_application_data_handler handler, void* user_context);        /* :201 */
CHARLS_AMD_API charls_jpegls_errc charls_decoder_get_compressed_data_format(
    const charls_jpegls_decoder* decoder, charls_compressed_data_format* compressed_data_format);           /* :215 */
CHARLS_AMD_API charls_jpegls_errc charls_decoder_get_mapping_table_id(const charls_jpegls_decoder* decoder,
                                                                      int32_t component_index, int32_t* table_id); /* :229 */
CHARLS_AMD_API charls_jpegls_errc charls_decoder_find_mapping_table_index(const charls_jpegls_decoder* decoder,
                                                                          int32_t mapping_table_id, int32_t* index); /* :244 */
CHARLS_AMD_API charls_jpegls_errc charls_decoder_get_mapping_table_count(const charls_jpegls_decoder* decoder,
                                                                         int32_t* count);                   /* :257 */
CHARLS_AMD_API charls_jpegls_errc charls_decoder_get_mapping_table_info(const charls_jpegls_decoder* decoder,
                                                                        int32_t mapping_table_index,
                                                                        charls_mapping_table_info* mapping_table_info); /* :273 */
CHARLS_AMD_API charls_jpegls_errc charls_decoder_get_mapping_table_data(const charls_jpegls_decoder* decoder,
                                                                        int32_t mapping_table_index,
                                                                        void* mapping_table_data,
                                                                        size_t mapping_table_size_bytes);   /* :291 */

/* ------------------------------------------------------------------------------------------------------------------
 * Part 1c -- misc: include/charls/jpegls_error.h:12, jpegls_error.hpp:10, version.h:43-54, validate_spiff_header.h:23
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API const char* charls_get_error_message(charls_jpegls_errc error_value);
CHARLS_AMD_API const void* charls_get_jpegls_category(void); /* really `const std::error_category*`, as in the reference */
CHARLS_AMD_API const char* charls_get_version_string(void);
CHARLS_AMD_API void charls_get_version_number(int32_t* major, int32_t* minor, int32_t* patch);
CHARLS_AMD_API charls_jpegls_errc charls_validate_spiff_header(const charls_spiff_header* spiff_header,
                                                               const charls_frame_info* frame_info);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2 -- additive batch API on DEVICE memory (no reference counterpart; never changes part 1 semantics).
 *
 * A batch is `frame_count` independent frames with identical coding parameters.  Frame f's pixels start at
 * d_frames + f * frame_pitch_bytes in the reference's user layout (planar for ILV_NONE, pixel-interleaved otherwise,
 * `stride` bytes between rows, 0 = minimal).  Frame f's complete .jls file is produced at / read from
 * d_streams + f * stream_pitch_bytes.  `sizes` and `errcs` are HOST arrays of frame_count elements.
 * `hip_stream` is a hipStream_t (NULL = default stream); the calls return after the stream work has completed.
 * Every frame gets the bytes and the errc the part-1 encoder/decoder would give it with a destination buffer of
 * stream_pitch_bytes (encode) or a source buffer of sizes[f] bytes (decode).
 * Slots need no alignment, but the decoders load whole 16-byte aligned groups: the device allocation that holds
 * d_streams must be readable from the 16-byte boundary at or before its first slot to the one at or after the end of its
 * last slot (any hipMalloc'ed buffer is; a slot that ends on the last byte of a sub-allocated pool may not be).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct charls_amd_codec_params
{
    charls_frame_info frame_info;
    int32_t near_lossless;
    charls_interleave_mode interleave_mode;
    charls_color_transformation color_transformation;
    charls_jpegls_pc_parameters preset_coding_parameters; /* all zero = defaults */
    charls_encoding_options encoding_options;
    uint32_t restart_interval; /* lines per restart interval, 0 = none (encode: extension below; decode: from DRI) */
} charls_amd_codec_params;

CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_device(const charls_amd_codec_params* params,
                                                                 uint32_t frame_count, const void* d_frames,
                                                                 size_t frame_pitch_bytes, uint32_t stride,
                                                                 void* d_streams, size_t stream_pitch_bytes,
                                                                 uint64_t* sizes, charls_jpegls_errc* errcs,
                                                                 void* hip_stream);

CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device(uint32_t frame_count, const void* d_streams,
                                                                 size_t stream_pitch_bytes, const uint64_t* sizes,
                                                                 void* d_frames, size_t frame_pitch_bytes,
                                                                 uint32_t stride, charls_amd_codec_params* params_out,
                                                                 charls_jpegls_errc* errcs, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2b -- several GPUs from one process (frames are the sharding unit; no exchange while coding; the only
 * collective is the hand-over of the finished bitstreams).  The frames of a batch are dealt to shards; shard s lives on
 * device shards[s].device with its frames and its stream slots in that device's memory, at the pitches given to the call.
 * A worker thread per shard, bound to the shard's device, runs charls_amd_encode_batch_device / _decode_batch_device on the
 * shard (the threads belong to a context that lives across calls, see charls_amd_devices below); sizes / errcs are HOST arrays over all frames in shard order (shard 0's frames first).  Every frame gets exactly
 * the bytes and the errc of part 1, whatever the number of shards.
 *
 * encode, gather != NULL: after coding, every shard's streams are brought together, back to back and in frame order, in
 * gather->d_gathered on the device of shard gather->root_shard; offsets[f] is where frame f starts (frames that failed
 * take no room), *total_bytes the end.  The sizes are exchanged first (a prefix sum over host values here), then every
 * other shard sends each stream -- exactly sizes[f] bytes -- to its place: with RCCL (ncclSend / ncclRecv pairs in groups,
 * point to point over xGMI; librccl.so is opened at run time) or with peer copies (hipMemcpyPeerAsync).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct charls_amd_device_shard
{
    int32_t device;       /* HIP device ordinal */
    uint32_t frame_count; /* frames of this shard (may be 0) */
    const void* d_frames; /* encode: source frames; decode: destination frames (written) */
    void* d_streams;      /* encode: destination slots; decode: source slots */
    void* hip_stream;     /* a hipStream_t of that device, or NULL */
} charls_amd_device_shard;

typedef enum charls_amd_transport
{
    CHARLS_AMD_TRANSPORT_AUTO = 0,       /* RCCL when it can be loaded and the shards sit on distinct devices, else peer copies */
    CHARLS_AMD_TRANSPORT_RCCL = 1,       /* fail when RCCL is not usable */
    CHARLS_AMD_TRANSPORT_PEER_COPIES = 2
} charls_amd_transport;

typedef struct charls_amd_gather
{
    uint32_t root_shard;
    void* d_gathered;      /* on the root shard's device */
    size_t capacity_bytes;
    uint64_t* offsets;     /* HOST, one per frame */
    uint64_t* total_bytes; /* HOST, may be NULL */
    charls_amd_transport transport;
} charls_amd_gather;

CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_devices(const charls_amd_codec_params* params,
                                                                  uint32_t shard_count, const charls_amd_device_shard* shards,
                                                                  size_t frame_pitch_bytes, uint32_t stride,
                                                                  size_t stream_pitch_bytes, uint64_t* sizes,
                                                                  charls_jpegls_errc* errcs, const charls_amd_gather* gather);

CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_devices(uint32_t shard_count, const charls_amd_device_shard* shards,
                                                                  size_t stream_pitch_bytes, const uint64_t* sizes,
                                                                  size_t frame_pitch_bytes, uint32_t stride,
                                                                  charls_amd_codec_params* params_out, charls_jpegls_errc* errcs);

/* The context behind the two calls above.  It lives across calls and owns a worker thread per (device, shard ordinal on
 * that device), bound to its device for life -- the encoder's work areas belong to the thread that made them, so a second
 * call of the same shape allocates nothing -- and the RCCL communicator and exchange streams of the last gathered call
 * (re-made only when the list of devices changes).  One call at a time per context; different contexts are independent.
 * charls_amd_encode_batch_devices / charls_amd_decode_batch_devices run on a process-wide default context, which is also
 * what a NULL `context` argument means below; charls_amd_devices_destroy(NULL) releases everything the default context
 * holds (its threads end, their work areas are freed, the communicator is destroyed). */
typedef struct charls_amd_devices charls_amd_devices;
CHARLS_AMD_API charls_amd_devices* charls_amd_devices_create(void); /* NULL when out of memory */
CHARLS_AMD_API void charls_amd_devices_destroy(charls_amd_devices* context);
CHARLS_AMD_API charls_jpegls_errc charls_amd_devices_encode_batch(charls_amd_devices* context, const charls_amd_codec_params* params,
                                                                  uint32_t shard_count, const charls_amd_device_shard* shards,
                                                                  size_t frame_pitch_bytes, uint32_t stride,
                                                                  size_t stream_pitch_bytes, uint64_t* sizes,
                                                                  charls_jpegls_errc* errcs, const charls_amd_gather* gather);
CHARLS_AMD_API charls_jpegls_errc charls_amd_devices_decode_batch(charls_amd_devices* context, uint32_t shard_count,
                                                                  const charls_amd_device_shard* shards, size_t stream_pitch_bytes,
                                                                  const uint64_t* sizes, size_t frame_pitch_bytes, uint32_t stride,
                                                                  charls_amd_codec_params* params_out, charls_jpegls_errc* errcs);
CHARLS_AMD_API uint64_t charls_amd_devices_work_area_bytes(charls_amd_devices* context); /* HBM held by the context's workers */
CHARLS_AMD_API charls_jpegls_errc charls_amd_devices_release_work_areas(charls_amd_devices* context); /* (the threads stay) */

/* Extension: restart intervals on the encoder of part 1.  `lines` rows per interval (0 = none, the default) are coded
 * independently -- by different wavefronts at the same time -- and separated by RSTm markers; a DRI segment announces
 * the interval.  The reference's encoder has no equivalent (its output never contains restart markers); its decoder
 * reads these streams (reference src/jpeg_stream_reader.cpp:586-607, src/scan_decoder.hpp:335-349), and this library's
 * decoder decodes the intervals in parallel.  Must be called before the first encode_* call of an image. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_encoder_set_restart_interval(charls_jpegls_encoder* encoder,
                                                                                 uint32_t lines);

/* Extension: the seek-point index of the decoder of part 1.  A JPEG-LS decoder's state at a line boundary is
 * small and complete (the contexts, RUNindex, the previous line, the bit position); saved every K lines during one decode,
 * it lets a later decode of the same stream start one wavefront per K lines -- interval-parallel decoding of streams that
 * have no restart markers -- and decode a band of rows without the rows above the seek point before it.
 * The index is a portable sidecar (little-endian, no pointers; layout: charls_amd/csrc/host/seek_index.h): a header that
 * names K and the frame (width, height, bits, components, interleave mode, NEAR, T1..T3, RESET, color transformation),
 * then per scan the length and a 64-bit hash of its entropy-coded segment and its seek points.  Scans the exact decoder
 * does not take (lines beyond its LDS, RESET = 256 m), scans with restart intervals (already parallel) and frames whose
 * height comes from DNL get no seek points and decode the ordinary way.
 *
 * get_index_size: after read_header; an upper bound of the index's bytes for K = lines_per_seek_point (>= 1).
 * decode_to_buffer_and_index: decode_to_buffer (same pixels, errc and state transition) that also writes the index to
 *   `index` and its size to *index_bytes; slower than a plain decode (one wavefront per scan, as the exact decoder).  An
 *   index_capacity below get_index_size is invalid_argument_size, checked before anything is decoded; nothing is written
 *   to `index` when the decode fails.  Indexed calls launch on their own: they are not merged with other threads' calls.
 * set_index: after read_header; copies the index after checking its format, the frame it names and the range of every
 *   field of every seek point (a forged or truncated index can make a decode slower, never make a kernel read or write
 *   out of bounds).  invalid_argument, and nothing kept, on any mismatch.  Needs no GPU.  decode_to_buffer then decodes
 *   every scan that has seek points as intervals that start from them, and accepts the result only when every interval
 *   ends in exactly the state the next seek point claims (by induction from the true initial state the output is then
 *   exact, whatever the index holds); a scan whose segment hash differs or whose chain does not hold is decoded from the
 *   top (charls_amd_index_counters [2]).
 * decode_rows: after read_header, and leaves the handle there (one handle can decode many bands).  Rows
 *   [first_row, first_row + row_count) in decode_to_buffer's layout for a frame of row_count rows (planar frames: one band
 *   per component, back to back; stride 0 = packed).  With an index the decode of each scan starts at the seek point at or
 *   before first_row; a band cannot be checked by chaining, so the index is TRUSTED once its segment hash matches the
 *   stream (invalid_argument otherwise): set only an index that was built from this stream.  Without an index the decode
 *   starts at the top on the exact decoder (~1.3 MPix/s for one stream: a band far down a large frame then takes longer
 *   than decode_to_buffer, which runs on the faster group decoder).  Either way it stops after the band: damage inside or above the band gives the exact decoder's errc,
 *   damage below it is not looked at.  Scans without seek points (restart intervals, the cases above) are decoded whole on
 *   the ordinary path and the band is copied out. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_decoder_get_index_size(const charls_jpegls_decoder* decoder,
                                                                           uint32_t lines_per_seek_point, size_t* bytes);
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_decoder_decode_to_buffer_and_index(
    charls_jpegls_decoder* decoder, void* destination_buffer, size_t destination_size_bytes, uint32_t stride,
    uint32_t lines_per_seek_point, void* index, size_t index_capacity, size_t* index_bytes);
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_decoder_set_index(charls_jpegls_decoder* decoder, const void* index,
                                                                      size_t index_size_bytes);
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_decoder_decode_rows(charls_jpegls_decoder* decoder, uint32_t first_row,
                                                                        uint32_t row_count, void* destination_buffer,
                                                                        size_t destination_size_bytes, uint32_t stride);
/* What the seek-point index did since the library was loaded (process-wide): out[0] scans decoded from seek points (full
 * decodes and bands), out[1] wavefronts launched from the index (intervals and bands), out[2] scans whose index did not
 * hold (hash or chain check) and that were decoded from the top, out[3] launches of the seek kernels (the one that writes
 * seek points and the one that starts from them; a batch call of part 2c is one launch per group of scans, not one per
 * frame).  Returns the number of values written (4 at most; a caller that asks for 3 gets the first three). */
CHARLS_AMD_API int32_t charls_amd_index_counters(uint64_t* out, int32_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2c -- the seek-point index in the batch API: streams, frames and bands are DEVICE memory as in part 2, indexes are
 * HOST memory (they are sidecars that come from and go to storage; checking one needs no GPU).  Index f lies at
 * indexes + f * index_pitch_bytes; index_sizes is a HOST array of frame_count elements.
 *
 * The contract per frame is part 1's: frame f gets the pixels, the index bytes and the errc that a fresh part-1 decoder
 * gives for the same stream -- set_source_buffer(stream f, sizes[f]), read_header, set_index where there is one, then
 * decode_to_buffer_and_index, decode_to_buffer or decode_rows --, errcs[f] being the first code of that sequence that is
 * not success.  In particular: an index_pitch_bytes below the frame's get_index_size is invalid_argument_size and nothing
 * of that frame is decoded; an index set_index would refuse is invalid_argument; a full decode through an index is kept
 * only when every interval ends in exactly the next seek point's state, and is otherwise done again from the top
 * (charls_amd_index_counters [2]); a band trusts an index whose segment hash matches and is invalid_argument otherwise;
 * frames that get no seek points (restart intervals, scans the exact decoder does not take, a height from DNL, a scan
 * whose parameters differ from the first scan's) go the ordinary way.  16-bit frames whose rows would start at odd addresses
 * (an odd d_frames / d_bands, pitch or stride) go the ordinary way too and get an index without seek points.
 * One frame's failure never changes another frame's result, and nothing is written outside a frame's own extent of
 * d_frames, d_bands or indexes.  The return value, hip_stream, stride, params_out and the 16-byte readability rule for
 * d_streams are those of charls_amd_decode_batch_device; the frames of a call may differ in geometry and coding
 * parameters.  The segment hashes are computed on the device: no stream is copied to the host.
 *
 * All scans of a call that share the seek kernels' specialisation (sample width, components per pixel) are ONE launch:
 * building runs one launch per group and scan ordinal (scan c + 1 starts where scan c ended); decoding through indexes
 * and decoding bands run one launch per group for all scans of all frames (the index names every segment's length).
 * Frames whose chain check fails and frames without seek points are decoded in the same call by the ordinary launches.
 *
 * index_size_bound: what get_index_size returns for a stream with these parameters (an upper bound of the index for
 *   K = lines_per_seek_point >= 1); needs no GPU.  encoding_options is not looked at.
 * decode_batch_device_and_index: charls_amd_decode_batch_device that also builds every frame's index; index_sizes[f] is
 *   its size, 0 where the frame failed (nothing is written to its slot then).
 * decode_batch_device_indexed: charls_amd_decode_batch_device through indexes; index_sizes[f] == 0: frame f has no index
 *   and decodes the ordinary way.  Worth it for small batches: see INTEGRATION.md.
 * decode_rows_batch_device: rows [first_rows[f], first_rows[f] + row_counts[f]) of frame f in decode_rows' layout at
 *   d_bands + f * band_pitch_bytes (a band_pitch_bytes below what the band needs: invalid_argument_size for that frame).
 *   index_sizes[f] == 0: from the top.  Frames without seek points, and planar frames without an index, are decoded whole
 *   into a work area on the ordinary path and the band is copied out (damage below the band is then reported too).
 * These three take fixed-pitch slots and one frame pitch; part 2l has them on a packed blob with a destination per frame, and
 * an index-only build that needs no frames at all. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_index_size_bound(const charls_amd_codec_params* params,
                                                              uint32_t lines_per_seek_point, size_t* bytes);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_and_index(
    uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes, const uint64_t* sizes, void* d_frames,
    size_t frame_pitch_bytes, uint32_t stride, uint32_t lines_per_seek_point, void* indexes, size_t index_pitch_bytes,
    uint64_t* index_sizes, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_indexed(
    uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes, const uint64_t* sizes, const void* indexes,
    size_t index_pitch_bytes, const uint64_t* index_sizes, void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
    charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_rows_batch_device(
    uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes, const uint64_t* sizes, const void* indexes,
    size_t index_pitch_bytes, const uint64_t* index_sizes, const uint32_t* first_rows, const uint32_t* row_counts,
    void* d_bands, size_t band_pitch_bytes, uint32_t stride, charls_jpegls_errc* errcs, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2d -- PACKED streams in the batch API: the streams of a batch back to back in ONE device buffer with a HOST table
 * of offsets -- the form files, archives, DICOM multi-frame pixel data and charls_amd_gather hold them in -- instead of
 * fixed-pitch slots.  Frame f's .jls is the sizes[f] bytes at d_packed + offsets[f].  `offsets`, `sizes` and `errcs` are HOST
 * arrays; the return value, hip_stream, stride and params_out are those of part 2.  New entry points beside the slot
 * calls: those and the multi-device calls of part 2b stay on slots; the indexed calls of part 2c take packed streams in
 * part 2l.
 *
 * The offset rule (pack_streams, encode_batch_device_packed): offsets[0] = 0 and offsets[f + 1] = offsets[f] + sizes[f]
 * rounded up to `offset_alignment`, a power of two in [1, 4096] (anything else: invalid_argument for the whole call, before
 * anything is done).  The alignment is of the offset within d_packed, not of the address.  The bytes of the gaps are
 * zero.  A frame with sizes[f] == 0 -- a frame that failed -- takes no room, as in charls_amd_gather.  offsets has
 * frame_count + 1 elements; offsets[frame_count] is the total.
 *
 * pack_streams_device: the slot array of charls_amd_encode_batch_device (frame f at d_streams + f * stream_pitch_bytes,
 *   sizes[f] bytes) into the packed form, with one launch of a copy kernel that takes any alignment on either side.  A
 *   sizes[f] above stream_pitch_bytes, or a total beyond packed_capacity_bytes, is invalid_argument_size and nothing is
 *   written, neither to d_packed nor to offsets.  d_streams and d_packed must not overlap.  The copy loads whole 16-byte
 *   aligned groups: the readability rule of part 2 holds for d_streams.
 * encode_batch_device_packed: frame f gets exactly the bytes and the errc charls_amd_encode_batch_device gives it with
 *   stream_pitch_bytes = max_stream_bytes (0 = charls_jpegls_encoder_get_estimated_destination_size of the frame; too small
 *   a value is destination_too_small for the frames it is too small for, as there), placed at offsets[f] under the rule
 *   above with sizes[f] == 0 for every frame whose errc is not success.  The capacity: a frame whose end offsets[f] +
 *   sizes[f] lies beyond packed_capacity_bytes gets destination_too_small, and so does EVERY frame after it; nothing of
 *   them is written and they take no room.  Nothing is written at or beyond packed_capacity_bytes (the zeros behind the
 *   last frame that fits stop there, though offsets[f + 1] follows the rule).  The caller provides no slots: the call codes
 *   passes of frames into staging slots of its own and packs every pass with one launch.  The staging slots are one more
 *   work area of the calling thread (at most a quarter of what its work areas may hold, see
 *   charls_amd_set_workspace_limit; counted by charls_amd_work_area_bytes, freed by charls_amd_release_work_areas); when
 *   not even one slot of max_stream_bytes can be had the call returns not_enough_memory.
 * decode_batch_device_packed: charls_amd_decode_batch_device with frame f's stream at d_packed + offsets[f] (offsets has
 *   frame_count elements): the same pixels, params_out and errcs, for frames of mixed geometry and coding parameters, for
 *   damaged and truncated streams; one frame's failure never changes another's.  The offsets may come in any order, at
 *   any alignment, and may name the same bytes twice (streams are only read).  offsets[f] + sizes[f] that overflows is
 *   invalid_argument_size for the whole call.  Readability: the allocation that holds d_packed must be readable from the
 *   16-byte boundary at or before the lowest offset to the one at or after the highest end (any hipMalloc'ed buffer is).
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_errc charls_amd_pack_streams_device(uint32_t frame_count, const void* d_streams,
                                                                 size_t stream_pitch_bytes, const uint64_t* sizes,
                                                                 void* d_packed, size_t packed_capacity_bytes,
                                                                 uint32_t offset_alignment, uint64_t* offsets, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_device_packed(
    const charls_amd_codec_params* params, uint32_t frame_count, const void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
    void* d_packed, size_t packed_capacity_bytes, uint32_t offset_alignment, size_t max_stream_bytes, uint64_t* offsets,
    uint64_t* sizes, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_packed(uint32_t frame_count, const void* d_packed,
                                                                        const uint64_t* offsets, const uint64_t* sizes,
                                                                        void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
                                                                        charls_amd_codec_params* params_out,
                                                                        charls_jpegls_errc* errcs, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2e -- RAGGED frames in the batch API: the frames of ONE call may differ in geometry and coding parameters and need
 * not share an allocation -- archives, DICOM studies with several series, tile grids with edge tiles (a tile is a pointer
 * into the image with the image's row length as its stride), thumbnails beside full frames, lists of separately allocated
 * tensors.  Every frame brings a table entry of its own; streams are in the packed form of part 2d on both sides (a caller
 * who has slots passes offsets[f] = f * pitch).  `sources`, `dests`, `offsets`, `sizes`, `errcs`, `params_out` and
 * `frame_bytes_out` are HOST arrays of frame_count elements (encode: offsets has frame_count + 1); the return value and
 * hip_stream are those of part 2.  New entry points beside the existing ones, none of which changes.  `reserved` must be 0.
 *
 * probe_batch_device_packed: what the streams of a packed blob hold, WITHOUT decoding them -- a caller sizes and allocates
 *   its destinations from it.  errcs[f] is the first code that is not success from a fresh part-1 decoder's
 *   set_source_buffer(stream f, sizes[f]) and read_header; on success params_out[f] holds what
 *   charls_amd_decode_batch_device_packed reports for the frame and frame_bytes_out[f] what
 *   charls_jpegls_decoder_get_destination_size(stride 0) returns; on failure both are zeroed (as they are for an abbreviated
 *   table-only stream, on which read_header succeeds).  The first bytes of every stream are gathered on the device and
 *   brought over in one copy, as the batch decoders do it; no whole stream is copied to the host and no decoder is launched.
 *   The readability rule of part 2d applies to d_packed.
 * decode_batch_device_ragged: per frame the pixels, params_out[f] (an ARRAY here; zeroed for a frame that did not get as
 *   far as its first scan) and the errc of charls_amd_decode_batch_device_packed, frame f going to dests[f].d_pixels with
 *   dests[f].stride.  A stride below the frame's row is invalid_argument_stride for that frame; a capacity_bytes below
 *   stride * rows - (stride - row) is invalid_argument_size for that frame (rows: the rows of all planes of a planar
 *   frame).  Both are checked against the whole frame once its header is read: neither affects another frame, nothing of a
 *   frame that fails them is written, and nothing is written outside any frame's extent.  The destinations may sit in
 *   different allocations; destinations that overlap are the caller's error and are not looked for.  A d_pixels of NULL with
 *   a capacity_bytes that is not 0, or a `reserved` that is not 0, is invalid_argument for the whole call.
 * encode_batch_device_ragged: frame f gets exactly the bytes and the errc charls_amd_encode_batch_device_packed gives a
 *   batch that holds this one frame, with sources[f].params, .stride and .max_stream_bytes, placed by the offset rule of
 *   part 2d IN THE CALLER'S FRAME ORDER.  The capacity rule is the same: a frame whose end lies beyond
 *   packed_capacity_bytes gets destination_too_small and so does every frame after it in the caller's order, whatever order
 *   they were coded in.  Parameters the encoder refuses (2 > bits, a color transformation with NEAR, a stride below the
 *   row, ...) are THAT FRAME's errc, with sizes[f] == 0 and no room taken -- not the call's return value.  Errors of the
 *   whole call, checked before anything is done: NULL tables, a `reserved` that is not 0, a d_pixels of NULL, an
 *   offset_alignment that is no power of two in [1, 4096].  The same pixels may be named by several frames.
 *   How: the frames are walked in the caller's order in WINDOWS; inside a window the frames with equal params, stride and
 *   max_stream_bytes form a group, every group is coded by the launches of charls_amd_encode_batch_device into a stretch of
 *   staging slots of its own, and the whole window is packed by ONE launch of the copy kernel, the running offset carrying
 *   from window to window.  The staging is the work area of charls_amd_encode_batch_device_packed under its rule (a quarter
 *   of what the thread's work areas may hold; not_enough_memory when a configured workspace limit does not cover the
 *   largest frame's slot).  Not done: the groups of a window run one after another, not on side streams; the
 *   multi-device calls of part 2b stay as they are (the indexed calls of part 2c take ragged frames in part 2l); the tile pipeline has no mixed-geometry launch (a
 *   batch of many geometries with few frames each pays one set of launches per geometry and window).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct charls_amd_frame_source /* encode: one frame of a ragged batch */
{
    charls_amd_codec_params params; /* this frame's own parameters */
    const void* d_pixels;           /* first row, the reference's user layout for params */
    uint32_t stride;                /* 0 = minimal */
    uint32_t reserved;              /* must be 0 */
    uint64_t max_stream_bytes;      /* 0 = part 1's estimated destination size of this frame */
} charls_amd_frame_source;

typedef struct charls_amd_frame_dest /* decode: where one frame goes */
{
    void* d_pixels;
    uint64_t capacity_bytes; /* bytes the call may write from d_pixels on */
    uint32_t stride;         /* 0 = minimal */
    uint32_t reserved;       /* must be 0 */
} charls_amd_frame_dest;

CHARLS_AMD_API charls_jpegls_errc charls_amd_probe_batch_device_packed(uint32_t frame_count, const void* d_packed,
                                                                       const uint64_t* offsets, const uint64_t* sizes,
                                                                       charls_amd_codec_params* params_out,
                                                                       uint64_t* frame_bytes_out, charls_jpegls_errc* errcs,
                                                                       void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_ragged(uint32_t frame_count, const void* d_packed,
                                                                        const uint64_t* offsets, const uint64_t* sizes,
                                                                        const charls_amd_frame_dest* dests,
                                                                        charls_amd_codec_params* params_out,
                                                                        charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_device_ragged(uint32_t frame_count, const charls_amd_frame_source* sources,
                                                                        void* d_packed, size_t packed_capacity_bytes,
                                                                        uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes,
                                                                        charls_jpegls_errc* errcs, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2f -- encoding to a BYTE BUDGET.  JPEG-LS has no rate control: the size of a frame at some NEAR is known only once
 * it has been coded.  These calls walk the coding chains of every frame at every candidate NEAR in one launch that writes no
 * stream (K candidates of N frames cost K x N x scans results of 16 bytes, no stream slots), report the sizes, and code
 * every frame once, at the first candidate its budget allows.  Frames are uniform as in part 2 (frame f at d_frames +
 * f * frame_pitch_bytes, one params, one stride; not done here: ragged frames and streams as the source, which are part 2k);
 * params->near_lossless is not looked at.  `near_candidates`, `budgets`,
 * `sizes_out`, `offsets`, `sizes`, `near_out` and `errcs` are HOST arrays; candidate_count is 1 .. 64; the candidates may
 * come in any order and may repeat: the order given is the order of preference.
 *
 * measure_batch_device: sizes_out[f * candidate_count + c] is the sizes[f] that charls_amd_encode_batch_device_packed
 *   reports for frame f with near_lossless = near_candidates[c] and max_stream_bytes = 0 -- the complete .jls file, the
 *   even-size padding included -- without writing any stream (0 for a frame the encoder fails on at that NEAR).
 * encode_batch_device_budget: near_out[f] is the first candidate, in the order given, whose complete stream has at most
 *   budgets[f] bytes -- a limit on the size of the result, not a destination capacity with the reference's four-bytes-spare
 *   flush rule --, and frame f's bytes are exactly those charls_amd_encode_batch_device_packed produces with that
 *   near_lossless and max_stream_bytes = 0.  No candidate fits: errcs[f] = destination_too_small, near_out[f] = -1,
 *   sizes[f] = 0 and the frame takes no room.  Placement, offset_alignment, zeroed gaps and the capacity rule are those of
 *   part 2d (offsets has frame_count + 1 elements): a frame whose end lies beyond packed_capacity_bytes is
 *   destination_too_small (near_out[f] = -1), so is every frame after it, and nothing is written at or beyond the capacity.
 * Errors of the whole call, checked before a device is asked for and before anything is written: NULL tables or pointers, a
 *   candidate_count outside 1 .. 64, an offset_alignment that is no power of two in [1, 4096], and parameters the encoder
 *   refuses with ANY of the candidates (the return value is the code for the first such candidate: NEAR above the largest
 *   legal one, NEAR > 0 with a colour transformation, preset parameters invalid for that NEAR, ...).  frame_count == 0 is
 *   success.
 * How: the sizing launch is the group encoder's chain (contexts, run mode, reconstruction, Golomb code, bit writer with its
 *   0xFF rule) without a destination, laid out candidate-major with as few lanes per chain as the count of chains allows;
 *   the container bytes are added on the host.  The chosen (frame, NEAR) pairs are coded by
 *   charls_amd_encode_batch_device_ragged -- frames of one NEAR are one group -- into staging slots sized by the largest
 *   measured stream.  Scans the group encoder does not take (lines beyond LDS, charls_amd_set_encode_engine(1)) and frames
 *   with a restart interval are sized by coding them for real into the staging work area, candidate by candidate in the
 *   order given; the budget call stops at a frame's first candidate that fits, the measure call codes all of them.
 * measure_counters: out[0] scans sized by the measuring kernels, out[1] launches of them, out[2] scans sized by coding them
 *   for real; process-wide since load; returns the number of values written (3 at most).
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_errc charls_amd_measure_batch_device(const charls_amd_codec_params* params, uint32_t frame_count,
                                                                  const void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
                                                                  const int32_t* near_candidates, uint32_t candidate_count,
                                                                  uint64_t* sizes_out, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_device_budget(
    const charls_amd_codec_params* params, uint32_t frame_count, const void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
    const uint64_t* budgets, const int32_t* near_candidates, uint32_t candidate_count, void* d_packed, size_t packed_capacity_bytes,
    uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes, int32_t* near_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API int32_t charls_amd_measure_counters(uint64_t* out, int32_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2g -- SALVAGE decode: restart intervals confine damage.  charls_amd_decode_batch_device_ragged fails a frame as a
 * whole when one byte of it is damaged; a frame coded with a restart interval (DRI) consists of intervals that decode on
 * their own, and this call gives back the ones that are intact.  `reports` is a HOST array of frame_count elements,
 * `interval_status` a HOST array (may be NULL); everything else is the ragged call's.
 *
 * Round 1 is charls_amd_decode_batch_device_ragged, unchanged: the return value, params_out[f], errcs[f] and the pixels of
 *   every frame with errcs[f] == 0 are exactly that call's, for every input, and such a frame gets state 0.  A batch without
 *   failed frames launches nothing else (charls_amd_salvage_counters does not move).  Errors of the whole call are those of
 *   the ragged call and, checked before a device is asked for, `reports` == NULL and `interval_status` != NULL with
 *   status_pitch_bytes == 0.  frame_count == 0 is success.
 * Round 2 takes a frame with errcs[f] != 0 whose header was read and whose first scan was located, that passed its stride and
 *   capacity checks, and whose first scan has a restart interval below the frame's height, at most 65535 rows, and is a scan
 *   the interval-parallel decoder takes.  Every other failed frame gets state 2, counts of 0, and nothing is
 *   promised about its destination, as before.  errcs[f] stays what round 1 said -- state 1 is how a caller learns that the
 *   destination is usable -- with one exception: a fill_value above the frame's MAXVAL makes errcs[f] invalid_argument for a
 *   frame that would have been salvaged (state 2).
 * The segment of scan c runs from behind its SOS header to the first FF xx with xx >= 0x80 that is no FF D0..D7, or to the
 *   end of the source.  The markers FF D0+n inside it, m_0 .. m_{M-1} with numbers n_k, cut it into the pieces
 *   P_0 = [0, m_0), P_k = [m_{k-1} + 2, m_k), P_M = [m_{M-1} + 2, end).  N = ceil(height / Ri).  At most N + 7 markers are
 *   recorded; with more, the recorded ones count as all of them and q = 0.
 * Which piece is which interval -- never by guessing how many markers were lost:
 *   forward: p is the largest p <= min(M, N - 1) with n_k == k mod 8 for all k < p; piece k < p claims interval k.
 *   backward: q is the largest q <= min(M, N - 1) with n_{M-1-t} == (N - 2 - t) mod 8 for all t < q; piece M - t, t < q,
 *   claims interval N - 1 - t.  A piece with two different claims claims nothing; an interval claimed by two different pieces
 *   is claimed by none.  (Eight markers lost in a row cannot be seen in the 3-bit numbers: every piece between then has two
 *   claims, and nothing is misplaced.)
 * A claimed piece is decoded as an independent scan of that interval's rows.  The interval is KEPT if and only if the scan
 *   ends without error, leaves no decision open and consumed exactly the piece's bytes.  Every other interval is LOST: its
 *   rows get fill_value as the sample value of every component (16-bit samples little-endian), after the decoders have run.
 *   This is deliberately stricter than the reference's reader, which skips a pad byte or FF fill bytes in front of a marker:
 *   a piece that ends that way is lost here.  It only ever applies to frames that failed round 1.  Damage that decodes
 *   cleanly to the piece's exact length cannot be seen by anyone, here or in the reference.
 * Later scans of a planar frame: scan c + 1 is looked for where scan c's segment ends; if no valid SOS of a scan of the same
 *   kind is there, every interval of the scans not reached is lost and filled.
 * interval_status + f * status_pitch_bytes holds one byte per (scan, interval) of a salvaged frame, scan-major: 0 kept,
 *   1 no piece claimed the interval, 2 the piece did not decode to its exact length, 3 the scan was not reached.  A
 *   status_pitch_bytes below scans x N leaves that frame's status unwritten and sets reports[f].reserved to 1; the pixels
 *   and the report are valid all the same.
 * Nothing is written outside the rows of a frame's own destination; one frame's damage never changes another frame's result.
 * charls_amd_jpegls_decoder_decode_to_buffer_salvage: the same for one stream in host memory, after read_header.  It returns
 *   what charls_jpegls_decoder_decode_to_buffer returns; where that is an error and the report says state 1, `destination`
 *   holds the salvaged frame.  interval_status (may be NULL) has room for status_capacity bytes.  It launches on its own and
 *   stages through the handle's device buffers.
 * charls_amd_last_timings after the batch call: [0], [1] as after the ragged call; where a round 2 ran, [2] is the time that
 *   round took in ms by the host's clock (each of its launches ends in a synchronise).
 * salvage_counters: out[0] frames salvaged, out[1] intervals kept, out[2] intervals lost, out[3] launches of the salvage
 *   kernels; process-wide since load; returns the number of values written (4 at most).
 * Not done: partial intervals, the slot and multi-device calls.  Streams without restart intervals: part 2h.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct charls_amd_salvage_report
{
    uint32_t state;          /* 0 decoded whole; 1 salvaged; 2 failed and nothing salvaged; 3 (part 2h) the rows before the error */
    uint32_t intervals;      /* restart intervals of the frame, summed over its scans (state 1; else 0) */
    uint32_t intervals_lost;
    uint32_t rows_lost;      /* rows filled, summed over scans (a planar frame counts each plane's rows) */
    uint32_t first_lost_row; /* lowest row of the frame that holds fill in any scan; UINT32_MAX: none */
    uint32_t reserved;       /* written as 0 (bit 0: status_pitch_bytes was too small for this frame; bit 1, part 2h: its index was not usable) */
} charls_amd_salvage_report;

CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_salvage(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const charls_amd_frame_dest* dests,
    uint32_t fill_value, charls_amd_codec_params* params_out, charls_amd_salvage_report* reports, uint8_t* interval_status,
    size_t status_pitch_bytes, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_decoder_decode_to_buffer_salvage(
    charls_jpegls_decoder* decoder, void* destination, size_t size, uint32_t stride, uint32_t fill_value,
    charls_amd_salvage_report* report, uint8_t* interval_status, size_t status_capacity);
CHARLS_AMD_API int32_t charls_amd_salvage_counters(uint64_t* out, int32_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2h -- SALVAGE decode through the SEEK-POINT INDEX: streams without restart markers.  The reference's encoder never
 * writes restart markers, so part 2g helps none of the files it wrote.  A seek-point index (part 1 extension, part 2c) that
 * was built while the stream was sound holds the complete decoder state every K lines; it confines damage the same way.
 * Argument for argument the calls are part 2g's, with the indexes of part 2c (HOST; index_sizes[f] == 0: frame f has none;
 * `indexes` may be NULL when every size is 0) and `flags`: bit 0 CHARLS_AMD_SALVAGE_PREFIX, any other bit is
 * invalid_argument for the call.  The whole-call checks are part 2g's plus index_sizes == NULL, all made before a device is
 * asked for; frame_count == 0 is success.
 *
 * Round 1 is charls_amd_decode_batch_device_ragged, unchanged, exactly as in part 2g (state 0; a batch without failed frames
 *   launches nothing else; errcs[f] stays round 1's for salvaged frames, but for a fill_value above MAXVAL).
 * Round 2 takes a failed frame whose header was read, whose first scan was located, and which passed its stride and capacity
 *   checks:
 * 1. A frame part 2g salvages is salvaged exactly as there: the same report and status bytes, state 1.
 * 2. INDEX MODE (state 1): index_sizes[f] != 0, the index passes set_index's checks (format, the frame it names, every
 *   field's range) and has seek points for every scan, the scans are ones the seek kernels take (part 2c), the height does
 *   not come from DNL, and the rows of 16-bit frames lie at even addresses.  The segment hash is NOT consulted: it cannot
 *   match a damaged segment.  With K the index's lines and N = ceil(height / K), interval i of scan c covers rows
 *   [iK, min(height, (i+1)K)).  It starts from the scan's initial state at the segment start (i = 0) or from point i, and is
 *   KEPT if and only if it decodes without error and, for i < N-1, ends in exactly the state of point i+1 (the comparison
 *   part 1's chain check makes: contexts, run state, previous line, reader position and cache); for i = N-1, the scan ends
 *   and the bytes consumed equal the segment length the index names.  Every other interval is LOST: all of its rows get
 *   fill_value after the decoders have run -- rows decoded before the error too; nothing unverified is kept in this mode.
 *   An interval whose point puts the reader beyond the source bytes that are left is not started (status 3).  Scan c+1 of
 *   a planar frame is looked for at scan c's segment start plus the length the index names for it -- a damaged scan does not
 *   hide the ones behind it, as it does in part 2g; with no valid SOS of a scan of the same kind there, the intervals of that
 *   scan and of the scans behind it are not reached.
 *   Status bytes, one per (scan, interval), scan-major:
 *     0  kept, and so is every interval above it in the scan: exact whatever the index holds, by induction from the true
 *        initial state
 *     4  kept on the index's word: its start state came from a point that the chain no longer proves
 *     2  did not decode to the next point's state
 *     3  not reached
 *   STATUS 4 IS AS GOOD AS THE INDEX.  Set only an index that was built from this very stream while it was sound.  A wrong
 *   index loses intervals.  A forged one can give wrong pixels in status-4 intervals, but never a read or a write out of
 *   bounds.  An index that is refused or lacks points counts as absent; reports[f].reserved bit 1 (value 2) says so.
 * 3. PREFIX MODE (state 3): only with CHARLS_AMD_SALVAGE_PREFIX and no usable index, under the same conditions on scans and
 *   rows.  The frame is decoded from the top on the exact decoder.  Scan c fails after r complete rows: scans before c are
 *   whole, rows [0, r) of scan c are what the decoder produced, rows [r, height) of scan c and every later scan get
 *   fill_value.  One status byte per scan: 0 whole, 5 prefix, 3 not reached; `intervals` counts scans, intervals_lost those
 *   that are not whole, first_lost_row the lowest row that holds fill in any scan.  This is what the reference leaves in a
 *   caller's buffer.  It is right for truncated files and UNVERIFIED after a bit error: on a 70x40 8-bit frame of 1275
 *   bytes with 4 bytes zeroed in the middle the reference's decoder writes 38 rows before it raises invalid_data and only
 *   the first 19 equal the sound image (12-bit: 35 written, 19 right; 35x24 RGB line- and sample-interleaved: 22-23 written,
 *   11 right; cut in the middle and closed with FF D9: 19 written, all 19 right).  Rows behind a bit error are mostly
 *   garbage that nobody can tell from pixels; the index tells them apart and gives back what lies below the damage.
 * 4. Every other failed frame gets state 2, as in part 2g.
 * In every mode nothing is written outside the rows of a frame's own destination, and one frame's damage never changes
 *   another frame's result.
 * charls_amd_jpegls_decoder_decode_to_buffer_salvage_indexed: the same for one stream in host memory, after read_header and,
 *   optionally, set_index.  Returns what decode_to_buffer returns; with state 1 or 3 `destination` holds the salvaged frame.
 * charls_amd_last_timings after the batch call: [2] as in part 2g, covering everything behind round 1; [3] the launches of
 *   this part by device events, ms.
 * salvage_index_counters: out[0] frames salvaged by index, out[1] intervals kept proven (0), out[2] kept on the index (4),
 *   out[3] lost (2, 3), out[4] frames salvaged by prefix, out[5] kernel launches of this part (one of the resume kernel and
 *   one of the fill kernel per group of scans that share sample width, interleaving, geometry and K); process-wide since
 *   load; returns the number of values written (6 at most).
 * Not done: partial intervals in index mode, the slot and multi-device calls, building an index from a damaged stream.
 * ---------------------------------------------------------------------------------------------------------------- */
#define CHARLS_AMD_SALVAGE_PREFIX 1u

CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_salvage_indexed(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const void* indexes,
    size_t index_pitch_bytes, const uint64_t* index_sizes, const charls_amd_frame_dest* dests, uint32_t fill_value, uint32_t flags,
    charls_amd_codec_params* params_out, charls_amd_salvage_report* reports, uint8_t* interval_status, size_t status_pitch_bytes,
    charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_jpegls_decoder_decode_to_buffer_salvage_indexed(
    charls_jpegls_decoder* decoder, void* destination, size_t size, uint32_t stride, uint32_t fill_value, uint32_t flags,
    charls_amd_salvage_report* report, uint8_t* interval_status, size_t status_capacity);
CHARLS_AMD_API int32_t charls_amd_salvage_index_counters(uint64_t* out, int32_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2i -- the batch API on HOST memory: frames and streams in the caller's host memory, one call, the PCIe copies
 * overlapped with the coding inside it.  Every pointer below is a HOST pointer (the d_pixels members of
 * charls_amd_frame_source / charls_amd_frame_dest too); there is no hip_stream argument and the calls return when the
 * results are in the caller's memory.  The device is the calling thread's current device.  New entry points; nothing else
 * changes, and the multi-device calls of part 2b stay as they are.
 *
 * Results: frame for frame what the device calls of part 2e give on device copies of the same data -- the same offsets
 * (with the zeroed alignment gaps), sizes, stream bytes, errcs, params_out and pixels.  The capacity rule holds in the
 * caller's order: a frame whose end lies beyond packed_capacity_bytes is destination_too_small and so is every frame
 * behind it, whichever part of the batch was coded first.  One frame's failure changes no other frame's result.  Decode
 * writes only the row bytes of each destination -- stride padding and everything outside a frame's extent stay as they
 * were -- and nothing at all of a frame that fails; encode never writes to a source; nothing is written at or beyond
 * packed_capacity_bytes.
 * Whole-call errors are those of part 2e (NULL tables, a `reserved` that is not 0, a NULL pixel pointer, an
 * offset_alignment that is no power of two in [1, 4096]); all are found before a device is asked for, and nothing is
 * written then.  frame_count == 0 is success, with offsets[0] = 0 on encode.
 * Host memory of any kind works, mixed within one call, at any base address: memory pinned by charls_amd_host_alloc, by
 * charls_amd_host_register or by someone else's hipHostMalloc / hipHostRegister is copied from and to directly; pageable
 * memory goes through pinned staging buffers of the library (bounded: CHARLS_AMD_HOST_STAGE_BYTES per lane, 64 MiB by
 * default) at the price of one more copy on the host.
 * Threading: the calls may be made from several threads; calls on one device take turns.
 * How: the frames are walked in the caller's order in windows; a few LANES -- persistent worker threads of the library
 * bound to the device, each with a stream and buffers of its own -- serve the windows round-robin, so that one window's
 * copies run under another window's coding.  Encode brings the rows up packed (stride padding never crosses PCIe), codes a
 * window with charls_amd_encode_batch_device_ragged and brings its streams down with one copy; decode parses the headers on
 * the host, sends exactly sizes[f] bytes per stream, decodes with charls_amd_decode_batch_device_ragged and writes the rows
 * at the caller's stride.  Memory: what the lanes hold on the device -- frames, streams, and the work areas of the device
 * calls they make -- stays within charls_amd_set_workspace_limit, all lanes together; not_enough_memory when a configured
 * limit cannot hold the largest single frame.  charls_amd_release_work_areas also releases what the lanes hold, device and
 * pinned (the threads stay).  Knobs: HOST_LANES, HOST_WINDOW_FRAMES, HOST_STAGE_BYTES.
 *
 * host_alloc / host_free / host_register / host_unregister: pinned memory for callers without a HIP header.  Without a
 *   usable device: NULL / CHARLS_AMD_ERRC_DEVICE_UNAVAILABLE.  host_free(NULL) is a no-op.  Registering pins whole PAGES:
 *   register memory whose pages are the caller's alone (a mapping, a page-aligned allocation), not an object in the middle
 *   of a heap page that other objects share, and unregister it before the memory goes back to its allocator.
 * probe_batch_host_packed: the contract of charls_amd_probe_batch_device_packed on host bytes; needs no GPU, asks for none.
 * encode_batch_host_ragged / decode_batch_host_ragged: the calls of part 2e with host tables AND host data.
 * encode_batch_host / decode_batch_host: one geometry, frame f at frames + f * frame_pitch_bytes; the argument lists of
 *   charls_amd_encode_batch_device_packed / charls_amd_decode_batch_device_packed without hip_stream (params_out: ONE element).
 * host_counters, process-wide since the library was loaded: out[0] host batch calls, out[1] windows, out[2] bytes copied
 *   host to device, out[3] device to host, out[4] bytes of pageable caller memory that went through the staging buffers,
 *   out[5] device bytes the lanes hold now, out[6] pinned bytes the lanes hold now.  Returns the number of values (7 at most).
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API void* charls_amd_host_alloc(size_t size_bytes);
CHARLS_AMD_API void charls_amd_host_free(void* memory);
CHARLS_AMD_API charls_jpegls_errc charls_amd_host_register(void* memory, size_t size_bytes);
CHARLS_AMD_API charls_jpegls_errc charls_amd_host_unregister(void* memory);
CHARLS_AMD_API charls_jpegls_errc charls_amd_probe_batch_host_packed(uint32_t frame_count, const void* packed, const uint64_t* offsets,
                                                                     const uint64_t* sizes, charls_amd_codec_params* params_out,
                                                                     uint64_t* frame_bytes_out, charls_jpegls_errc* errcs);
CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_host_ragged(uint32_t frame_count, const charls_amd_frame_source* sources,
                                                                      void* packed, size_t packed_capacity_bytes, uint32_t offset_alignment,
                                                                      uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_host_ragged(uint32_t frame_count, const void* packed, const uint64_t* offsets,
                                                                      const uint64_t* sizes, const charls_amd_frame_dest* dests,
                                                                      charls_amd_codec_params* params_out, charls_jpegls_errc* errcs);
CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_host(const charls_amd_codec_params* params, uint32_t frame_count,
                                                               const void* frames, size_t frame_pitch_bytes, uint32_t stride, void* packed,
                                                               size_t packed_capacity_bytes, uint32_t offset_alignment,
                                                               size_t max_stream_bytes, uint64_t* offsets, uint64_t* sizes,
                                                               charls_jpegls_errc* errcs);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_host(uint32_t frame_count, const void* packed, const uint64_t* offsets,
                                                               const uint64_t* sizes, void* frames, size_t frame_pitch_bytes, uint32_t stride,
                                                               charls_amd_codec_params* params_out, charls_jpegls_errc* errcs);
CHARLS_AMD_API int32_t charls_amd_host_counters(uint64_t* out, int32_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2j -- RE-CODING the streams of a packed blob in one call.  Only this library's encoder writes restart intervals; the
 * streams callers already hold -- archives written by the reference, DICOM multi-frame pixel data -- have none, so they decode
 * as one dependency chain each and part 2g cannot confine damage in them.  This call decodes every stream of a blob and codes
 * it again with a few parameters replaced -- a restart interval added, NEAR raised for an archive tier -- without the caller
 * owning the frames in between.  `offsets_in`, `sizes_in`, `specs`, `offsets_out` (frame_count + 1), `sizes_out`,
 * `params_out` and `errcs` are HOST arrays; the blobs are DEVICE memory; the return value and hip_stream are those of part 2.
 * specs: ONE element for every frame (spec_count == 1) or one per frame (spec_count == frame_count).
 *
 * The contract is a composition, byte for byte.  Frame f's output is what charls_amd_encode_batch_device_ragged writes for one
 * source whose pixels are what charls_amd_decode_batch_device_ragged decodes from input stream f into a packed destination
 * (stride 0), whose params are that decode's params_out[f] with the fields named by specs[f].set replaced, and whose
 * max_stream_bytes is 0; params_out[f] is what the frame was coded with.  Placement is part 2d's offset rule in the caller's
 * order, zeroed gaps included, and part 2d's capacity rule holds: a frame whose end lies beyond packed_capacity_bytes gets
 * destination_too_small with sizes_out[f] == 0, and so does EVERY frame behind it in the caller's order, whatever it holds
 * (those frames need not be decoded; params_out[f] is then the stream's parameters with the spec where its header can be
 * read, else zeroed).  Nothing is written at or beyond packed_capacity_bytes.
 * Failures of a frame: one whose decode fails keeps the decoder's code in errcs[f], has sizes_out[f] == 0, takes no room and
 *   gets a zeroed params_out[f]; one the encoder refuses (a colour transformation with NEAR above 0, preset parameters that are
 *   invalid for the frame, ...) gets the encoder's code.  One frame's failure never changes another frame's bytes, nor the
 *   offset arithmetic beyond taking no room.
 * Errors of the whole call, all checked before a device is asked for, nothing being written: NULL tables or blobs, a
 *   spec_count that is neither 1 nor frame_count, a `set` bit that is not defined, a `reserved` that is not 0, an
 *   offset_alignment that is no power of two in [1, 4096] (invalid_argument), an offsets_in[f] + sizes_in[f] that overflows
 *   (invalid_argument_size).  frame_count == 0 is success with offsets_out[0] == 0.  The input and the output must not
 *   overlap; this is not looked for.  The readability rule of part 2d applies to d_packed_in.
 * What does not survive: the output container is the batch encoder's -- SOI, SOF55, LSE where the parameters are not the
 *   defaults, DRI, the scans, EOI.  SPIFF headers, comments and application-data segments of the source are dropped, and a
 *   height that came from a DNL segment is written into the frame header.  A frame one of whose scan headers names a mapping
 *   table (a table id that is not 0 for any component) is refused with invalid_operation once it has decoded: the batch
 *   encoder cannot write the table, and dropping the reference silently would change what the samples mean.
 *   With set == 0 a LOSSLESS stream in that plain container comes back byte for byte, and with a new restart interval its
 *   pixels are unchanged.  A near-lossless stream is coded near-lossless again: its pixels stay within its NEAR of what the
 *   input decodes to, and even with set == 0 its bytes may change (where a reconstructed sample was clamped at 0 or MAXVAL the
 *   second quantisation differs; the reference's encoder on the reference's decode does the same).
 * How: one probe of the whole batch gives every frame's size.  The frames are then walked in the caller's order in WINDOWS:
 *   the longest run of frames whose packed pixels, each frame rounded up to 256 bytes, fit one more work area of the calling
 *   thread (at most a quarter of what its work areas may hold, see charls_amd_set_workspace_limit; counted by
 *   charls_amd_work_area_bytes, freed by charls_amd_release_work_areas; the knob TRANSCODE_WINDOW_FRAMES forces the length).
 *   A configured workspace limit that does not cover the largest frame, or its staging slot in the encoder, makes the call
 *   return not_enough_memory before anything is written.  Per window: the ragged decode into the area, the ragged encode of
 *   the frames that decoded at d_packed_out + base with what is left of the capacity, and base added to the offsets; base is
 *   the end of the window before, a multiple of the alignment, so bytes, gaps and offsets are those of one encode over all
 *   frames.  A frame's header is parsed twice, by the probe and by its window's decode.
 * charls_amd_last_timings afterwards: [0] all launches, [1] their dominant kernels, [2] the decodes, [3] the encodes, ms.
 * transcode_batch_host: the same arguments with both blobs in HOST memory of any kind (part 2i: pinned memory is copied from
 *   and to directly, pageable memory goes through the lane's staging halves); the results are those of the device call on
 *   device copies of the same bytes.  Windows run one after another on ONE lane of part 2i -- the streams up into a 16-byte
 *   granular device window with its margin, the device call's body, the front of the window's blob down -- and nothing is
 *   pipelined: a window's PCIe traffic is two streams per frame, its decode a dependency chain per frame.  Knobs:
 *   HOST_WINDOW_FRAMES, HOST_STAGE_BYTES.
 * transcode_counters, process-wide since the library was loaded: out[0] frames re-coded, out[1] windows of the device
 *   call, out[2] frames refused for a mapping table, out[3] frames behind the one that met the capacity.  Returns the number
 *   of values written (4 at most).
 * Not done: the decode of window w + 1 does not run under the encode of window w (the group decoder takes 156 of a CU's
 *   160 KB of LDS: the tile kernels cannot sit beside it); the interleave mode cannot be changed; the multi-device calls of
 *   part 2b are not joined to it.  The byte budget of part 2f is joined to it in part 2k.
 * ---------------------------------------------------------------------------------------------------------------- */
#define CHARLS_AMD_TRANSCODE_NEAR 1u
#define CHARLS_AMD_TRANSCODE_RESTART_INTERVAL 2u
#define CHARLS_AMD_TRANSCODE_PRESET 4u
#define CHARLS_AMD_TRANSCODE_ENCODING_OPTIONS 8u
typedef struct charls_amd_transcode_spec
{
    uint32_t set; /* which fields below replace the source stream's value; any other bit: invalid_argument */
    int32_t near_lossless;
    uint32_t restart_interval; /* lines; 0 removes restart intervals */
    charls_jpegls_pc_parameters preset_coding_parameters;
    charls_encoding_options encoding_options;
    uint32_t reserved; /* must be 0 */
} charls_amd_transcode_spec;

CHARLS_AMD_API charls_jpegls_errc charls_amd_transcode_batch_device(
    uint32_t frame_count, const void* d_packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
    const charls_amd_transcode_spec* specs, uint32_t spec_count, void* d_packed_out, size_t packed_capacity_bytes,
    uint32_t offset_alignment, uint64_t* offsets_out, uint64_t* sizes_out, charls_amd_codec_params* params_out,
    charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_transcode_batch_host(
    uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
    const charls_amd_transcode_spec* specs, uint32_t spec_count, void* packed_out, size_t packed_capacity_bytes,
    uint32_t offset_alignment, uint64_t* offsets_out, uint64_t* sizes_out, charls_amd_codec_params* params_out,
    charls_jpegls_errc* errcs);
CHARLS_AMD_API int32_t charls_amd_transcode_counters(uint64_t* out, int32_t capacity);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2k -- BYTE BUDGETS for ragged frames and for re-coding: part 2f joined with part 2e and with part 2j.  "Every frame of
 * this archive at no more than N bytes" is one call; the caller neither sorts frames into geometry groups nor owns decoded
 * frames.  All tables are HOST arrays as in parts 2e, 2f and 2j; `offsets` / `offsets_out` have frame_count + 1 elements,
 * `sizes_out` of the measure call frame_count * candidate_count.  The candidates are ONE list for the whole call, 1 .. 64
 * entries in any order, possibly repeating; the order given is the order of preference.  New entry points beside the existing
 * ones, none of which changes; no kernel, instantiation or descriptor field was added for them.
 *
 * measure_batch_device_ragged: row f of sizes_out is what charls_amd_measure_batch_device reports for a batch that holds this
 *   one frame, with sources[f].params, .stride and .d_pixels; params.near_lossless is not looked at.  Where that call would
 *   refuse the frame as a whole call -- a candidate above the frame's largest legal NEAR, NEAR > 0 with a colour
 *   transformation, preset parameters invalid at some candidate, a stride below the row -- its return value is errcs[f] and the
 *   row is zeroed; no other frame is affected.
 * encode_batch_device_ragged_budget: frame f gets exactly the near_out, sizes, errcs and stream bytes that
 *   charls_amd_encode_batch_device_budget gives a batch holding this one frame with budgets[f], placed by the offset rule of
 *   part 2d in the caller's frame order with zeroed gaps.  No candidate fits: destination_too_small, near_out[f] == -1,
 *   sizes[f] == 0, no room taken.  Parameters the encoder refuses with ANY candidate: that code, with -1, 0 and no room, as in
 *   the measure call.  The capacity rule of part 2d: the frame whose end lies beyond packed_capacity_bytes is
 *   destination_too_small (near_out -1), so is every frame behind it in the caller's order, and nothing is written at or
 *   beyond the capacity.  The same pixels may be named by several frames, for example with different budgets.
 * transcode_batch_device_budget: a composition, as part 2j is.  Frame f's output is what encode_batch_device_ragged_budget
 *   writes for one source whose pixels are what charls_amd_decode_batch_device_ragged decodes from input stream f into a packed
 *   destination, whose params are that decode's params_out[f] with the fields named by specs[f].set replaced, and whose budget
 *   is budgets[f].  params_out[f] is what the frame was coded with: near_lossless == near_out[f].  For a frame that was not
 *   coded, near_out[f] == -1 and params_out[f] is the source's parameters with the spec applied where the header could be
 *   read, zeroed otherwise (the rule of part 2j).  A frame whose decode fails, a frame that names a mapping table, the offsets
 *   and the capacity rule "this frame and every frame behind it" are those of part 2j, unchanged.
 *   The candidates are relative to the DECODED pixels: re-coding a near-lossless source stacks its NEAR with the chosen one
 *   (a source of NEAR 2 re-coded at candidate 3 may be off by 5 from what was first coded), and candidate 0 keeps the
 *   source's loss, it does not undo it.
 *   The call re-codes EVERY frame it is given.  A caller who wants frames that are already within their budget left alone
 *   leaves them out of the call: it holds sizes_in.
 * transcode_batch_host_budget: the same arguments with both blobs in HOST memory and no hip_stream; the results are those of
 *   the device call on device copies of the same bytes.  It runs in windows on one lane, exactly as
 *   charls_amd_transcode_batch_host does, budgets and candidates passed through window by window.
 * Errors of the whole call, all checked before a device is asked for, nothing being written.  invalid_argument: NULL tables
 *   or blobs, a candidate_count outside 1 .. 64, an offset_alignment that is no power of two in [1, 4096], a `reserved` that
 *   is not 0, a d_pixels of NULL, a sources[f].max_stream_bytes that is not 0 (the budget is the limit), a spec_count that is
 *   neither 1 nor frame_count, a `set` bit that is not defined, a spec with CHARLS_AMD_TRANSCODE_NEAR set (the candidates
 *   decide NEAR).  invalid_argument_size: an offsets_in[f] + sizes_in[f] that overflows.  frame_count == 0 is success with
 *   offsets[0] == 0.
 * How: the frames are walked once; frames with equal params (NEAR aside) and equal stride are a GROUP, in any positions of the
 *   caller's order.  Every group is sized by what one uniform call of part 2f over its frames does -- ONE measuring launch
 *   for all its frames and candidates, and the same fallback of coding for real for scans the group encoder does not take
 *   and for restart intervals --, never one call per frame.  The chosen (frame, NEAR) pairs of the whole call -- of the whole
 *   window when re-coding -- go through one ragged encode of part 2e, whose staging slots are sized per group and NEAR by
 *   the largest measured stream, so that the frames of a group that chose the same NEAR stay one encode group.  Re-coding
 *   shares the probe, the window plan, the decode, the offset arithmetic and the capacity tail with part 2j; only the encode
 *   step of a window differs.  Work areas are those of parts 2d and 2j under their rules (a quarter of what the thread's work
 *   areas may hold; not_enough_memory, before anything is written, when a configured workspace limit cannot hold the largest
 *   frame or its staging slot; TRANSCODE_WINDOW_FRAMES forces the window length).
 * Counters: sizing launches, sized scans and scans coded for real count into charls_amd_measure_counters; re-coded frames,
 *   windows, table refusals and frames behind the capacity into charls_amd_transcode_counters.  charls_amd_last_timings after
 *   a transcode call: [0] all launches, [1] their dominant kernels, [2] the decodes, [3] sizing and encoding, ms.
 * As in part 2f the staging slots follow the MEASURED streams, not part 1's estimated destination size: a frame whose stream
 *   is longer than that estimate (noise coded losslessly) is coded here, where charls_amd_encode_batch_device_packed with
 *   max_stream_bytes = 0 reports destination_too_small for it.  The host form gives every frame of a window the smaller of
 *   budgets[f] and the longest stream the code can produce for its geometry (LIMIT bits per sample and the stuffing) as room
 *   in the window's device blob, so such frames are coded there as well; budgets far above the frames' sizes make its windows
 *   shorter, nothing else.  The not_enough_memory check that comes before anything is written covers the largest frame and
 *   part 1's estimate of its stream: with a configured workspace limit between that estimate and the staging slot of a
 *   measured stream that is longer, a later window can return not_enough_memory after earlier windows have written theirs.
 *   A stride of 0 and a stride that states the packed row are different groups: the frames are coded the same, in one launch
 *   more.
 * Not done: one measuring launch over mixed geometries (the ragged encoder has no such launch either: G groups cost G
 *   launches); copying through, instead of re-coding, frames that are already within budget; the interleave mode; the
 *   multi-device calls of part 2b; a budgeted encode from host pixels.
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_errc charls_amd_measure_batch_device_ragged(
    uint32_t frame_count, const charls_amd_frame_source* sources, const int32_t* near_candidates, uint32_t candidate_count,
    uint64_t* sizes_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_encode_batch_device_ragged_budget(
    uint32_t frame_count, const charls_amd_frame_source* sources, const uint64_t* budgets, const int32_t* near_candidates,
    uint32_t candidate_count, void* d_packed, size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets,
    uint64_t* sizes, int32_t* near_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_transcode_batch_device_budget(
    uint32_t frame_count, const void* d_packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
    const charls_amd_transcode_spec* specs, uint32_t spec_count, const uint64_t* budgets, const int32_t* near_candidates,
    uint32_t candidate_count, void* d_packed_out, size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets_out,
    uint64_t* sizes_out, int32_t* near_out, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_transcode_batch_host_budget(
    uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
    const charls_amd_transcode_spec* specs, uint32_t spec_count, const uint64_t* budgets, const int32_t* near_candidates,
    uint32_t candidate_count, void* packed_out, size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets_out,
    uint64_t* sizes_out, int32_t* near_out, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2l -- the SEEK-POINT INDEX on PACKED streams: part 2c joined with parts 2d, 2e and 2i.  The calls of part 2c take
 * fixed-pitch slots and a frame per stream; an ingest job that wants the sidecars of a blob had to copy every stream into a
 * slot, allocate a full frame per stream and throw the pixels away.  Here the streams are a packed blob with an offset
 * table (part 2d: frame f's .jls is the sizes[f] bytes at d_packed + offsets[f]; the readability rule of part 2d applies),
 * the destinations are the table of part 2e -- or there are none --, and the indexes are HOST memory at
 * indexes + f * index_pitch_bytes as in parts 2c and 2h.  `offsets`, `sizes`, `errcs`, `index_sizes`, `first_rows`,
 * `row_counts` and `params_out` are HOST arrays of frame_count elements; params_out is an ARRAY as in part 2e, may be NULL, and
 * is zeroed for a frame that did not get as far as its first scan.  New entry points beside the existing ones, none of which
 * changes.
 *
 * The contract per frame is part 2c's, which is part 1's.  The index bytes are byte for byte what
 * charls_amd_decode_batch_device_and_index and charls_amd_jpegls_decoder_decode_to_buffer_and_index write for the same stream
 * and K: an index built here is accepted by parts 1, 2c and 2h, and the reverse.  Pixels, bands and errcs are those of the
 * slot calls on the same bytes, and the checks of a destination are those of charls_amd_decode_batch_device_ragged: a
 * stride below the frame's row is invalid_argument_stride for that frame, a capacity_bytes below the frame (the band) is
 * invalid_argument_size for that frame, both are checked against the whole frame once its header is read, and nothing of a
 * frame that fails them is written.  An index_pitch_bytes below the frame's get_index_size is invalid_argument_size for that
 * frame: nothing of it is decoded and index_sizes[f] is 0.  One frame's failure never changes another frame's result, and
 * nothing is written outside a frame's own extent of its destination or index slot.
 *
 * Whole-call errors, all checked before a device is asked for and before anything is written: NULL tables,
 * lines_per_seek_point == 0, a `reserved` that is not 0, a d_pixels of NULL with a capacity_bytes that is not 0
 * (invalid_argument); offsets[f] + sizes[f] that overflows (invalid_argument_size).  frame_count == 0 returns success.
 *
 * index_batch_device_packed: builds every frame's index, K = lines_per_seek_point.  With `dests` it is
 *   charls_amd_decode_batch_device_and_index on the blob and the caller's destinations (a 16-bit frame at an odd address or
 *   stride gets its pixels and an index without seek points, as there).  With dests == NULL it is the INDEX-ONLY build:
 *   errcs[f] is the code the frame would get with a destination of minimal stride -- the stream is decoded in full, only the
 *   pixels have nowhere to go -- and no caller memory but indexes, index_sizes, params_out and errcs is written.  The frames
 *   that are all seek points go through the kernel that writes them without a pixel pointer: no frame is allocated for
 *   them (a 16-bit frame is never at an odd address here, so it gets its seek points).  The frames that get no seek points
 *   in part 2c (restart intervals, a height from DNL, a scan the exact decoder does not take, a later scan whose parameters
 *   differ from the first scan's) get the index without seek points that part 2c writes, and are decoded for their errc
 *   into scratch frames: one more work area of the calling thread, filled in windows within a quarter of what its work areas
 *   may hold (knob INDEX_WINDOW_FRAMES), counted by charls_amd_work_area_bytes and freed by charls_amd_release_work_areas; when
 *   not one such frame fits, those frames get not_enough_memory.
 * decode_batch_device_ragged_indexed: charls_amd_decode_batch_device_indexed on the blob, frame f going to dests[f]
 *   (index_sizes[f] == 0: frame f has no index and decodes the ordinary way, as does a frame whose index does not hold).
 * decode_rows_batch_device_ragged: charls_amd_decode_rows_batch_device on the blob: rows [first_rows[f], first_rows[f] +
 *   row_counts[f]) of frame f in decode_rows' layout at bands[f].d_pixels with bands[f].stride; a capacity_bytes below what the
 *   band needs is invalid_argument_size for that frame.  `indexes` may be NULL when every index_sizes[f] is 0.
 * index_batch_host: the index-only build with the blob in HOST memory of any kind (part 2i: pinned memory is copied from
 *   directly, pageable memory through the lane's staging); there is no hip_stream argument and the call returns when the
 *   results are there.  Results are those of the device call on a device copy of the same bytes.  Windows run one after
 *   another on ONE lane of part 2i, as those of charls_amd_transcode_batch_host do -- the streams go up into a 16-byte
 *   granular device window, the body of the device call runs on it, and nothing comes down but what that body returns to the
 *   host anyway (HOST_WINDOW_FRAMES forces the window length).
 *
 * charls_amd_index_counters and charls_amd_last_timings are those of part 2c: the launches of the seek kernels are one per
 * group of scans and scan ordinal (pass), whatever form the streams come in.
 * Not done: the multi-device calls of part 2b; a host form of the indexed decode and of the bands; seek points from the
 *   group decoder (the index-only build runs the exact decoder, one wavefront per scan).
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_errc charls_amd_index_batch_device_packed(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes,
    const charls_amd_frame_dest* dests /* NULL: index only */, uint32_t lines_per_seek_point, void* indexes,
    size_t index_pitch_bytes, uint64_t* index_sizes, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
    void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_batch_device_ragged_indexed(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const void* indexes,
    size_t index_pitch_bytes, const uint64_t* index_sizes, const charls_amd_frame_dest* dests,
    charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_rows_batch_device_ragged(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const void* indexes,
    size_t index_pitch_bytes, const uint64_t* index_sizes, const uint32_t* first_rows, const uint32_t* row_counts,
    const charls_amd_frame_dest* bands, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API charls_jpegls_errc charls_amd_index_batch_host(
    uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes, uint32_t lines_per_seek_point,
    void* indexes, size_t index_pitch_bytes, uint64_t* index_sizes, charls_amd_codec_params* params_out,
    charls_jpegls_errc* errcs);

/* ------------------------------------------------------------------------------------------------------------------
 * Part 2m -- ROW BANDS THROUGH RESTART MARKERS.  A stream with restart intervals (written by the encoders on request, or
 * by charls_amd_transcode_batch_device from a stream the caller holds) never has seek points, and
 * charls_amd_decode_rows_batch_device_ragged decodes every such frame whole, one frame at a time, to copy a band out of it.
 * A band of `rows` rows meets only the intervals j0 = first_row / Ri .. j1 = (first_row + rows - 1) / Ri of each scan, and an
 * interval is a scan of its own.  charls_amd_decode_rows_batch_device_ragged_markers is that call, argument for argument --
 * the same tables, the same whole-call checks, made before a device is asked for; frame_count == 0 is success --, with one
 * more route for the frames that can take it.  None of the existing calls changes.
 *
 * A frame goes the MARKER ROUTE when its header was read and its band passed the stride and capacity checks of the ragged
 * band call (a frame that fails them is written nowhere), its height does not come from DNL, index_sizes[f] == 0 or its
 * index has no seek points, every scan has the first scan's parameters and a restart interval Ri with 0 < Ri < height, and
 * every scan is one the interval-parallel decoder takes (not: lines beyond LDS, RESET = 256 m, 16-bit rows at an odd address
 * or stride).  Every other frame is handed, unchanged, to the body of charls_amd_decode_rows_batch_device_ragged.
 *
 * On the route the restart markers of all such scans of the call are found in one launch per scan ordinal (the component
 * scans of a planar frame each have their own markers; scan c + 1 is found behind the marker that ends scan c, nothing of
 * scan c is decoded for that), their count must be ceil(height / Ri) - 1 and the markers up to the band must count
 * RST0 .. RST7 cyclically.  The intervals the bands meet, of all frames, are decoded by the ordinary decoders in one launch per
 * kernel specialisation: an interval that lies inside the band straight to its rows of bands[f], an interval that sticks out
 * of it -- at most two per scan -- into one more work area of the calling thread (256-byte aligned per interval, within a
 * quarter of what the thread's work areas may hold, counted by charls_amd_work_area_bytes, freed by
 * charls_amd_release_work_areas), from which its wanted rows are copied.  Every band interval must end without error, decided,
 * and -- but for the scan's last -- exactly at its marker.  A frame that fails any of this, or for whose edges there is no
 * room, or when a per-call buffer of the route (descriptors, results, line scratch: not work areas) cannot be allocated,
 * goes through the body of charls_amd_decode_rows_batch_device_ragged in the same call, which decodes it from the top
 * and reports what the reference reports; rows of its band that the first attempt wrote are written again or left beside an
 * errc, as that call leaves them.
 *
 * CONTRACT.  On a stream that decodes whole, bands and errcs are byte for byte those of
 * charls_amd_decode_rows_batch_device_ragged.  The one deliberate difference: damage that lies in an interval the band does not
 * meet (or behind the last scan), and that leaves the marker count and the marker numbers in front of the band intact, is not
 * looked at -- the frame gets its band and errc 0, where the existing call fails the frame.  The indexed band path makes the
 * same promise ("damage below it is not looked at"); a caller that wants the whole stream judged uses the existing call.
 * Nothing is written outside a band's own rows, and one frame's failure never changes another frame's result.
 *
 * charls_amd_band_marker_counters, process-wide since the library was loaded: out[0] frames that took the marker route,
 * out[1] intervals decoded on it, out[2] frames that fell back after starting it, out[3] launches the route made: one marker
 * search per scan ordinal and one decode launch per kernel specialisation among the intervals (a launch of the exact decoder
 * behind a speed path, for intervals that did not end cleanly there, is not counted).  Returns the number of values written
 * (4 at most).  charls_amd_last_timings is that of the frames that
 * went the existing way.
 * Not done: part 1's decode_rows; the slot and host-memory forms; a sidecar of marker offsets, so that repeated bands of one
 *   stream skip the marker walk; a row window inside the decode kernels, which would remove the edge copies; stopping the
 *   marker walk at the marker the band needs (the walk has no per-scan parameter for it).
 * ---------------------------------------------------------------------------------------------------------------- */
CHARLS_AMD_API charls_jpegls_errc charls_amd_decode_rows_batch_device_ragged_markers(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const void* indexes,
    size_t index_pitch_bytes, const uint64_t* index_sizes, const uint32_t* first_rows, const uint32_t* row_counts,
    const charls_amd_frame_dest* bands, charls_jpegls_errc* errcs, void* hip_stream);
CHARLS_AMD_API int32_t charls_amd_band_marker_counters(uint64_t* out, int32_t capacity);

/* Engine selection for the lossless single-component encoder: 0 = automatic, 1 = force the one-wavefront-per-scan
 * kernel, 2 = force the parallel pipeline (returns invalid_argument when the scan is not eligible). Process-wide. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_set_encode_engine(int32_t engine);

/* HBM kept by the library for its own work areas (the lossless encoder's per-scan work area of 8 B per sample of up to 8
 * bits -- 10 B per wider sample -- plus the unstuffed stream, the private buffers of restart intervals).  The batch entry
 * points of part 2 keep them per calling thread and device (a thread that moves to another device gets new ones there);
 * they grow on demand and stay allocated between calls.  The limit is process-wide: 0 (the default) = a quarter of the
 * device's memory, and never more than what is free minus 8 GiB.  A batch larger than the limit allows is coded in several
 * passes; when not even one work area can be allocated the encoder falls back to its one-wavefront-per-scan kernel, which
 * needs none (counted: charls_amd_engine_counters [4]).
 *
 * The host-pointer encoder / decoder of part 1 (THREADING, as the reference: distinct handles are independent, callers
 * scale by threads x handles): calls that arrive together are merged into one kernel launch (charls_amd_engine_counters),
 * and the merged encoder launches of ALL threads run on ONE set of work areas per device -- a pool of 256 threads holds
 * one arena, not 256.  That set never grows beyond the limit nor beyond an eighth of the device's memory (larger batches
 * take more passes) and stays allocated between calls that follow each other: giving gigabytes back to the driver and
 * asking for them again costs seconds, and hipFree waits for every kernel on the device.  Handles share a process-wide pool
 * of device buffers, streams and pinned staging areas (idle sets of at most 512 MiB each, per device at most 18 GiB or the
 * limit, whichever is less: callers create a handle per image, creating these per handle costs more than coding a frame).
 * None of it stays for long: once no coding call of part 1 has run for two seconds (CHARLS_AMD_IDLE_RELEASE_MS; 0 = keep) the
 * shared set, the idle pool and every block whose hipFree had been put off are given back by a housekeeping thread of the
 * library (charls_amd_engine_counters [6] - [8]).  charls_amd_release_work_areas frees the calling thread's areas, the shared
 * set and the idle pool at once. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_set_workspace_limit(uint64_t bytes);
CHARLS_AMD_API charls_jpegls_errc charls_amd_release_work_areas(void);
CHARLS_AMD_API uint64_t charls_amd_work_area_bytes(void); /* the calling thread's + the shared set of part 1, currently allocated */

/* What the engine did with the calls of part 1 since the library was loaded (process-wide): out[0] scan submissions of
 * the host-pointer ABI, out[1] kernel launches they took, out[2] submissions that shared their launch with another call,
 * out[3] scans of the largest launch, out[4] scans the lossless pipeline was eligible for that were coded by the
 * one-wavefront kernel because no work area could be allocated, out[5] merged launches that ran out of memory and whose
 * calls were then run one by one, out[6] bytes of device memory in the idle pool of handle resources, out[7] bytes whose
 * hipFree has been put off (a decoder launch is running), out[8] how often the housekeeping thread gave memory back,
 * out[9] scans a speed-path decoder handed to the exact decoder (streams that are damaged or that end unusually; a valid
 * stream that is counted here lost its speed path).  Returns the number of values written (10 at most). */
CHARLS_AMD_API int32_t charls_amd_engine_counters(uint64_t* out, int32_t capacity);

/* Test and measurement knobs (charls_amd/csrc/device/knobs.h has the list: DECODE_GROUP, JOB_EVENTS, TILE_SAMPLES,
 * COALESCE, ...).  The environment (CHARLS_AMD_<NAME>) is read ONCE, when the first knob is looked at; after that only this
 * call changes a value.  `name` with or without the CHARLS_AMD_ prefix; `value` INT64_MIN clears the knob (the engine's own
 * rule applies again).  Process-wide, not synchronised with calls in flight.  invalid_argument for an unknown name. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_debug_set_knob(const char* name, int64_t value);

/* Milliseconds of GPU time (hipEvent) the last batch call on this thread spent in its kernels, by stage:
 * out[0] total, out[1] dominant kernel, out[2..7] stage breakdown. Returns the number of values. */
CHARLS_AMD_API int32_t charls_amd_last_timings(double* out, int32_t capacity);

/* The lossless encoder codes the chain of every context in JOBS that start from a guessed state and are checked against
 * their predecessors afterwards; a job whose guess was wrong is coded again from the true state, so the bytes
 * never depend on the guesses -- only the time does.  Process-wide totals since the library was loaded:
 * out[0] jobs of the regular chains, out[1] how many of them were coded again, out[2] / out[3] the same for the run
 * chain; out[4] segments of the event lists of the rarer run-interruption context that were walked from a guessed state,
 * out[5] scans whose list was walked again serially because such a guess was wrong.  Frames whose jobs are mostly coded
 * again (full-range noise) encode at the speed of one lane per chain: a caller can tell from these counters.  Returns the
 * number of values written (6 at most). */
CHARLS_AMD_API int32_t charls_amd_speculation_counters(uint64_t* out, int32_t capacity);

/* 0 when a gfx950 device is usable, otherwise CHARLS_AMD_ERRC_DEVICE_UNAVAILABLE. */
CHARLS_AMD_API charls_jpegls_errc charls_amd_device_status(void);

#ifdef __cplusplus
}
#endif
#endif
