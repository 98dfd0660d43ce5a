// decoder_index.cpp -- the seek-point index of the decoder of part 1 (seek_index.h): building it during a
// decode, checking an index the caller hands in, decoding a scan through it, and decoding a band of rows.
//
// Trust model: a full decode through an index is accepted only when every interval ends in exactly the state the next
// seek point claims; by induction from the true initial state the output is then what the sequential decoder computes,
// whatever the index holds.  Anything else is decoded from the top on the ordinary path.  A band cannot be checked that
// way: decode_rows trusts an index whose segment hash matches the stream.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "../device/seek_decode.h"
#include "common.h"
#include "scan_engine.h"
#include "seek_index.h"
#include "segment_hash.h"

namespace jls {

namespace {

std::atomic<uint64_t> g_scans_from_points{0};
std::atomic<uint64_t> g_intervals{0};
std::atomic<uint64_t> g_fallbacks{0};
std::atomic<uint64_t> g_launches{0};

constexpr char kMagic[8] = {'J', 'L', 'S', 'S', 'E', 'E', 'K', '\0'};

template <typename T>
T load(const uint8_t* p) noexcept
{
    T v;
    std::memcpy(&v, p, sizeof v); // (the library runs on little-endian hosts only, as the device does)
    return v;
}
template <typename T>
void store(uint8_t* p, T v) noexcept
{
    std::memcpy(p, &v, sizeof v);
}

int32_t planes_of(const ScanSpec& s) noexcept
{
    return s.interleave_mode == 0 ? 1 : s.components;
}

} // namespace

bool seek_spec_eligible(const ScanSpec& s) noexcept
{
    return dev::seek_decode_eligible(desc_of(s)); // (device rows are packed: no odd row address for 16-bit samples)
}

bool same_scan_parameters(const ScanSpec& a, const ScanSpec& b) noexcept
{
    return a.components == b.components && a.interleave_mode == b.interleave_mode && a.near_lossless == b.near_lossless &&
           a.color_transformation == b.color_transformation && a.restart_interval == b.restart_interval &&
           std::memcmp(&a.pc, &b.pc, sizeof a.pc) == 0;
}

ScanSpec scan_spec_of(const StreamReader& r)
{
    const charls_frame_info& f = r.frame_info();
    return ScanSpec{f.width,
                    f.height,
                    static_cast<int32_t>(r.scan_component_count()),
                    r.parameters().interleave_mode,
                    f.bits_per_sample,
                    r.parameters().near_lossless,
                    r.parameters().transformation,
                    r.validated_pc(),
                    r.parameters().restart_interval};
}

size_t row_bytes_of(const ScanSpec& s) noexcept
{
    return static_cast<size_t>(planes_of(s)) * s.width * bytes_per_sample(s.bits_per_sample);
}
size_t seek_point_bytes(const ScanSpec& s) noexcept
{
    return seek::point_bytes(s.width, planes_of(s), s.bits_per_sample > 8);
}
size_t scans_of_frame(const StreamReader& r) noexcept
{
    return r.scan_interleave_mode() == 0 ? r.component_count() : 1;
}

charls_amd_codec_params params_of(const StreamReader& r)
{
    return charls_amd_codec_params{r.frame_info(), r.parameters().near_lossless, r.scan_interleave_mode(), r.parameters().transformation,
                                   r.preset_coding_parameters(), 0, r.parameters().restart_interval};
}

RowStride row_and_stride(const StreamReader& r, size_t stride_arg) noexcept
{
    const charls_frame_info& f = r.frame_info();
    const size_t row = (r.scan_interleave_mode() == 0 ? 1u : r.scan_component_count()) * static_cast<size_t>(f.width) * bytes_per_sample(f.bits_per_sample);
    return RowStride{row, stride_arg != 0 ? stride_arg : row};
}

namespace {

uint32_t expected_points(const StreamReader& r, const ScanSpec& first, uint32_t lines) noexcept
{
    return !r.height_from_dnl() && seek_spec_eligible(first) ? seek::points_per_scan(first.height, lines) : 0u;
}

// One seek point against the ranges a true decoder state keeps (A.12/A.13 and the kernel's packed forms): so that a forged
// point can cost time, never a read or write out of bounds.
bool point_in_range(const uint8_t* p, const ScanSpec& s, uint64_t segment_bytes) noexcept
{
    const int reset = static_cast<uint8_t>(s.pc.reset_value);
    const int maxval = (1 << s.bits_per_sample) - 1;
    for (uint32_t i = 0; i < seek::kCtxCount; ++i)
    {
        const uint32_t a = load<uint32_t>(p + seek::kCtxOff + 8 * i);
        const uint32_t bcn = load<uint32_t>(p + seek::kCtxOff + 8 * i + 4);
        const int minus_b = static_cast<int>(bcn & 0xFFu);
        const int c = static_cast<int>(static_cast<int8_t>((bcn >> 8) & 0xFFu));
        const int n = static_cast<int>(bcn >> 16);
        if (n < 1 || n > reset || minus_b >= n || c < -128 || c > 127 || a >= (1u << 24)) // (A halves down to 0 where errors are 0)
            return false;
    }
    for (int j = 0; j < 2; ++j)
    {
        const uint8_t* r = p + seek::kRunOff + 16 * j;
        const int32_t ritype = load<int32_t>(r), a = load<int32_t>(r + 4), n = load<int32_t>(r + 8), nn = load<int32_t>(r + 12);
        if (ritype != j || a < 0 || a > (1 << 25) || n < 1 || n > reset || nn < 0 || nn > n) // (run A halves down to 0)
            return false;
    }
    for (int j = 0; j < 4; ++j)
    {
        const int32_t run_index = load<int32_t>(p + seek::kRunIndexOff + 4 * j);
        const int32_t corner = load<int32_t>(p + seek::kCornerOff + 4 * j);
        if (run_index < 0 || run_index > 31 || corner < 0 || corner > maxval)
            return false;
    }
    if (load<uint32_t>(p + seek::kRestartOff) != 0 || load<uint32_t>(p + seek::kRestartOff + 4) != 0)
        return false; // (scans with restart intervals have no seek points)
    const bool wide = s.bits_per_sample > 8;
    const size_t samples = static_cast<size_t>(planes_of(s)) * (static_cast<size_t>(s.width) + 2);
    for (size_t i = 0; i < samples; ++i)
    {
        const int v = wide ? load<uint16_t>(p + seek::kLineOff + 2 * i) : p[seek::kLineOff + i];
        if (v > maxval)
            return false;
    }
    const uint8_t* rd = p + seek::reader_off(s.width, planes_of(s), wide);
    const uint64_t pos = load<uint64_t>(rd);
    const uint64_t valid = load<uint64_t>(rd + 16);
    return pos <= segment_bytes && valid <= 64;
}

} // namespace

uint64_t segment_hash(const uint8_t* p, size_t n) noexcept
{
    return segment_hash_bytes(p, n);
}

void index_counters(uint64_t out[4]) noexcept
{
    out[0] = g_scans_from_points.load();
    out[1] = g_intervals.load();
    out[2] = g_fallbacks.load();
    out[3] = g_launches.load();
}

void add_index_counters(uint64_t scans_from_points, uint64_t intervals, uint64_t fallbacks, uint64_t launches) noexcept
{
    g_scans_from_points.fetch_add(scans_from_points);
    g_intervals.fetch_add(intervals);
    g_fallbacks.fetch_add(fallbacks);
    g_launches.fetch_add(launches);
}

size_t index_size_bound(const ScanSpec& first, size_t scans, bool height_from_dnl, uint32_t lines)
{
    check_argument(lines > 0);
    const uint32_t points = !height_from_dnl && seek_spec_eligible(first) ? seek::points_per_scan(first.height, lines) : 0u;
    return kIndexHeaderBytes + scans * (kIndexScanBytes + points * seek_point_bytes(first));
}

size_t index_size_bound(const StreamReader& reader, uint32_t lines)
{
    return index_size_bound(scan_spec_of(reader), scans_of_frame(reader), reader.height_from_dnl(), lines);
}

SeekIndex parse_index(const StreamReader& reader, const uint8_t* data, size_t bytes)
{
    check_argument(data != nullptr && bytes >= kIndexHeaderBytes);
    check_argument(std::memcmp(data, kMagic, sizeof kMagic) == 0 && load<uint32_t>(data + 8) == kIndexVersion);
    const ScanSpec first = scan_spec_of(reader);
    const charls_frame_info& f = reader.frame_info();
    SeekIndex index;
    index.lines = load<uint32_t>(data + 12);
    check_argument(index.lines > 0);
    const uint32_t scans = load<uint32_t>(data + 60);
    check_argument(load<uint32_t>(data + 16) == f.width && load<uint32_t>(data + 20) == f.height &&
                   load<int32_t>(data + 24) == f.bits_per_sample && load<int32_t>(data + 28) == f.component_count &&
                   load<int32_t>(data + 32) == first.interleave_mode && load<int32_t>(data + 36) == first.near_lossless &&
                   load<int32_t>(data + 40) == first.pc.threshold1 && load<int32_t>(data + 44) == first.pc.threshold2 &&
                   load<int32_t>(data + 48) == first.pc.threshold3 && load<int32_t>(data + 52) == first.pc.reset_value &&
                   load<int32_t>(data + 56) == first.color_transformation && scans == scans_of_frame(reader) &&
                   load<uint32_t>(data + 64) == seek_point_bytes(first) && load<uint32_t>(data + 68) == 0);
    const uint32_t expected = expected_points(reader, first, index.lines);
    const size_t point_bytes = seek_point_bytes(first);
    check_argument(bytes >= kIndexHeaderBytes + scans * kIndexScanBytes);
    size_t at = kIndexHeaderBytes + scans * kIndexScanBytes;
    index.scans.resize(scans);
    for (uint32_t c = 0; c < scans; ++c)
    {
        const uint8_t* rec = data + kIndexHeaderBytes + c * kIndexScanBytes;
        IndexScan& s = index.scans[c];
        s.segment_bytes = load<uint64_t>(rec);
        s.hash = load<uint64_t>(rec + 8);
        s.points = load<uint32_t>(rec + 16);
        check_argument((s.points == 0 || s.points == expected) && load<uint32_t>(rec + 20) == 0);
        // (a segment longer than the source is not refused here: the decode finds the hash does not hold, and a damaged or
        // truncated stream then reports what the plain decoder reports)
        const size_t need = static_cast<size_t>(s.points) * point_bytes;
        check_argument(bytes - at >= need);
        for (uint32_t i = 0; i < s.points; ++i)
            check_argument(point_in_range(data + at + i * point_bytes, first, s.segment_bytes));
        s.data.assign(data + at, data + at + need);
        at += need;
    }
    check_argument(at == bytes);
    return index;
}

size_t write_index(const StreamReader& reader, const SeekIndex& index, uint8_t* out, size_t capacity)
{
    const ScanSpec first = scan_spec_of(reader);
    const charls_frame_info& f = reader.frame_info();
    size_t total = kIndexHeaderBytes + index.scans.size() * kIndexScanBytes;
    for (const IndexScan& s : index.scans)
        total += s.data.size();
    check_argument(total <= capacity, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    std::memset(out, 0, kIndexHeaderBytes);
    std::memcpy(out, kMagic, sizeof kMagic);
    store<uint32_t>(out + 8, kIndexVersion);
    store<uint32_t>(out + 12, index.lines);
    store<uint32_t>(out + 16, f.width);
    store<uint32_t>(out + 20, f.height);
    store<int32_t>(out + 24, f.bits_per_sample);
    store<int32_t>(out + 28, f.component_count);
    store<int32_t>(out + 32, first.interleave_mode);
    store<int32_t>(out + 36, first.near_lossless);
    store<int32_t>(out + 40, first.pc.threshold1);
    store<int32_t>(out + 44, first.pc.threshold2);
    store<int32_t>(out + 48, first.pc.threshold3);
    store<int32_t>(out + 52, first.pc.reset_value);
    store<int32_t>(out + 56, first.color_transformation);
    store<uint32_t>(out + 60, static_cast<uint32_t>(index.scans.size()));
    store<uint32_t>(out + 64, static_cast<uint32_t>(seek_point_bytes(first)));
    size_t at = kIndexHeaderBytes + index.scans.size() * kIndexScanBytes;
    for (size_t c = 0; c < index.scans.size(); ++c)
    {
        const IndexScan& s = index.scans[c];
        uint8_t* rec = out + kIndexHeaderBytes + c * kIndexScanBytes;
        store<uint64_t>(rec, s.segment_bytes);
        store<uint64_t>(rec + 8, s.hash);
        store<uint32_t>(rec + 16, s.points);
        store<uint32_t>(rec + 20, 0);
        if (!s.data.empty())
            std::memcpy(out + at, s.data.data(), s.data.size());
        // (the kernel writes a point's samples, not the bytes that pad its line to 8: they are zero in the file, whatever the
        // device buffer held, so that one stream has one index)
        const size_t point_bytes = seek_point_bytes(first);
        const size_t raw = static_cast<size_t>(planes_of(first)) * (static_cast<size_t>(first.width) + 2) * (first.bits_per_sample > 8 ? 2 : 1);
        const size_t pad = seek::line_bytes(first.width, planes_of(first), first.bits_per_sample > 8) - raw;
        for (size_t i = 0; pad != 0 && i < s.points && (i + 1) * point_bytes <= s.data.size(); ++i)
            std::memset(out + at + i * point_bytes + seek::kLineOff + raw, 0, pad);
        at += s.data.size();
    }
    return total;
}

size_t decode_scan_indexed(ScanEngine& engine, const ScanSpec& spec, const ScanSpec& first, size_t stream_offset, const uint8_t* segment,
                           size_t segment_left, uint8_t* destination, size_t stride, size_t scan_no, IndexMode mode, SeekIndex& index,
                           bool seek_allowed)
{
    const bool eligible = seek_allowed && same_scan_parameters(spec, first) && engine.seek_eligible(spec);
    if (mode == IndexMode::build)
    {
        if (index.scans.size() <= scan_no)
            index.scans.resize(scan_no + 1);
        IndexScan& s = index.scans[scan_no];
        s.points = eligible ? seek::points_per_scan(spec.height, index.lines) : 0u;
        s.data.assign(static_cast<size_t>(s.points) * seek_point_bytes(spec), 0);
        const size_t used = s.points != 0 ? engine.decode_scan_emit(spec, stream_offset, destination, stride, index.lines, s.data.data())
                                          : engine.decode_scan(spec, stream_offset, destination, stride);
        s.segment_bytes = used;
        s.hash = segment_hash(segment, used);
        return used;
    }
    if (mode == IndexMode::use && scan_no < index.scans.size() && index.scans[scan_no].points != 0)
    {
        const IndexScan& s = index.scans[scan_no];
        size_t used = 0;
        if (eligible && s.segment_bytes <= segment_left && segment_hash(segment, s.segment_bytes) == s.hash &&
            engine.decode_scan_resumed(spec, stream_offset, destination, stride, index.lines, s.data.data(), used))
            return used;
        g_fallbacks.fetch_add(1);
    }
    return engine.decode_scan(spec, stream_offset, destination, stride);
}

void decode_rows(const StreamReader& reader, ScanEngine& engine, const SeekIndex* index, uint32_t first_row, uint32_t row_count,
                 uint8_t* destination, size_t destination_size, size_t stride_arg)
{
    const charls_frame_info& f = reader.frame_info();
    check_argument(row_count > 0 && first_row < f.height && row_count <= f.height - first_row);
    const ScanSpec first = scan_spec_of(reader);
    const size_t scans = scans_of_frame(reader);
    const size_t row_bytes = row_bytes_of(first);
    const size_t stride = stride_arg == 0 ? row_bytes : stride_arg;
    check_argument(stride >= row_bytes, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE);
    const size_t needed = checked_mul(checked_mul(stride, row_count), scans) - (stride - row_bytes);
    check_argument(destination_size >= needed, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);

    const uint8_t* base = reader.position();
    StreamReader probe = reader;
    probe.at_comment(nullptr, nullptr);
    probe.at_application_data(nullptr, nullptr);
    engine.upload_stream(base, reader.remaining(), frame_hint(f.width, f.height, f.bits_per_sample));
    for (size_t c = 0; c < scans; ++c)
    {
        const ScanSpec spec = scan_spec_of(probe);
        const size_t offset = static_cast<size_t>(probe.position() - base);
        uint8_t* dst = destination + stride * row_count * c;
        const uint8_t* points = nullptr;
        if (index != nullptr && c < index->scans.size() && index->scans[c].points != 0)
        { // a band cannot be checked by chaining: the index must belong to this very segment
            const IndexScan& s = index->scans[c];
            check_argument(s.segment_bytes <= probe.remaining() && segment_hash(probe.position(), s.segment_bytes) == s.hash);
            if (same_scan_parameters(spec, first))
                points = s.data.data();
        }
        if (!reader.height_from_dnl() && engine.seek_eligible(spec))
        {
            engine.decode_scan_band(spec, offset, dst, stride, first_row, row_count, points != nullptr ? index->lines : 0, points);
        }
        else
        { // restart intervals, lines beyond LDS, RESET = 256 m, DNL: the whole scan on the ordinary path, the band copied
            std::vector<uint8_t> whole(row_bytes * f.height);
            (void)engine.decode_scan(spec, offset, whole.data(), row_bytes);
            for (uint32_t r = 0; r < row_count; ++r)
                std::memcpy(dst + stride * r, whole.data() + row_bytes * (first_row + r), row_bytes);
        }
        if (c + 1 == scans)
            break;
        // the next scan starts behind the first marker that is not a restart marker (FF followed by a byte >= 0x80 cannot
        // occur inside entropy-coded data)
        const uint8_t* p = probe.position();
        const uint8_t* end = p + probe.remaining();
        for (;; ++p)
        {
            p = static_cast<const uint8_t*>(std::memchr(p, 0xFF, static_cast<size_t>(end - p)));
            if (p == nullptr || p + 1 >= end)
                raise(CHARLS_JPEGLS_ERRC_NEED_MORE_DATA);
            if (p[1] >= 0x80 && !(p[1] >= 0xD0 && p[1] <= 0xD7))
                break;
        }
        probe.advance(static_cast<size_t>(p - probe.position()));
        probe.read_next_start_of_scan();
    }
}

// ---- ScanEngine's part (its resources; scan_engine.cpp does not know these calls)

bool ScanEngine::seek_eligible(const ScanSpec& spec) const
{
    return seek_spec_eligible(spec);
}

size_t ScanEngine::decode_scan_emit(const ScanSpec& spec, size_t stream_offset, uint8_t* destination, size_t stride, uint32_t lines,
                                    uint8_t* points)
{
    ensure_stream();
    const size_t row_bytes = row_bytes_of(spec);
    const size_t point_bytes = seek_point_bytes(spec);
    const size_t point_total = static_cast<size_t>(seek::points_per_scan(spec.height, lines)) * point_bytes;
    ScanDesc d = desc_of(spec);
    d.pixels = static_cast<uint8_t*>(r_->pixels.ensure(row_bytes * spec.height));
    d.pixel_stride = row_bytes;
    d.stream = r_->bits.as<uint8_t>() + stream_offset;
    d.stream_capacity = stream_bytes_ - stream_offset;
    d.line_scratch = nullptr; // (the wave decoder keeps its lines in LDS)
    auto* d_points = static_cast<uint8_t*>(r_->seek_points.ensure(std::max<size_t>(point_total, 16)));
    auto* d_desc = static_cast<ScanDesc*>(r_->desc.ensure(dev::with_headroom(sizeof(ScanDesc))));
    auto* d_result = static_cast<ScanResult*>(r_->result.ensure(dev::with_headroom(sizeof(ScanResult))));
    dev::hip_check(hipMemcpyAsync(d_desc, &d, sizeof d, hipMemcpyHostToDevice, r_->stream));
    dev::long_kernel_begins();
    try
    {
        dev::launch_seek_emit(d, d_desc, d_result, 1, d_points, 0, lines, r_->stream);
        g_launches.fetch_add(1);
    }
    catch (...)
    {
        dev::long_kernel_ends();
        throw;
    }
    ScanResult r{};
    const hipError_t copied = hipMemcpyAsync(&r, d_result, sizeof r, hipMemcpyDeviceToHost, r_->stream);
    const hipError_t synced = hipStreamSynchronize(r_->stream);
    dev::long_kernel_ends();
    dev::hip_check(copied);
    dev::hip_check(synced);
    if (r.errc != kOk)
        raise(static_cast<charls_jpegls_errc>(r.errc));
    copy_rows_out(destination, stride, d.pixels, row_bytes, spec.height);
    copy_out(points, d_points, point_total);
    return r.bytes;
}

bool ScanEngine::decode_scan_resumed(const ScanSpec& spec, size_t stream_offset, uint8_t* destination, size_t stride, uint32_t lines,
                                     const uint8_t* points, size_t& used)
{
    ensure_stream();
    const size_t row_bytes = row_bytes_of(spec);
    const size_t point_bytes = seek_point_bytes(spec);
    const uint32_t count = seek::points_per_scan(spec.height, lines);
    const uint32_t intervals = count + 1;
    ScanDesc d = desc_of(spec);
    d.pixels = static_cast<uint8_t*>(r_->pixels.ensure(row_bytes * spec.height));
    d.pixel_stride = row_bytes;
    d.stream = r_->bits.as<uint8_t>() + stream_offset;
    d.stream_capacity = stream_bytes_ - stream_offset;
    d.line_scratch = nullptr;
    std::vector<seek::SeekWork> work(intervals);
    for (uint32_t i = 0; i < intervals; ++i)
    {
        seek::SeekWork& w = work[i];
        w.scan = 0;
        w.first_row = i * lines;
        w.end_row = std::min(spec.height, (i + 1) * lines);
        w.store_from = w.first_row;
        w.row_base = 0;
        w.mode = i + 1 < intervals ? seek::kResumeCompare : seek::kResumeEnd;
        w.from_point = i == 0 ? 0 : (i - 1) * point_bytes;
        w.to_point = i + 1 < intervals ? i * point_bytes : 0;
    }
    const size_t point_total = static_cast<size_t>(count) * point_bytes;
    auto* d_points = static_cast<uint8_t*>(r_->seek_points.ensure(std::max<size_t>(point_total, 16)));
    auto* d_work = static_cast<seek::SeekWork*>(r_->seek_work.ensure(dev::with_headroom(sizeof(seek::SeekWork) * intervals)));
    auto* d_desc = static_cast<ScanDesc*>(r_->desc.ensure(dev::with_headroom(sizeof(ScanDesc))));
    auto* d_results = static_cast<ScanResult*>(r_->result.ensure(dev::with_headroom(sizeof(ScanResult) * intervals)));
    dev::hip_check(hipMemcpyAsync(d_points, points, point_total, hipMemcpyHostToDevice, r_->stream));
    dev::hip_check(hipMemcpyAsync(d_work, work.data(), sizeof(seek::SeekWork) * intervals, hipMemcpyHostToDevice, r_->stream));
    dev::hip_check(hipMemcpyAsync(d_desc, &d, sizeof d, hipMemcpyHostToDevice, r_->stream));
    dev::launch_seek_resume(d, d_desc, d_work, d_results, intervals, d_points, r_->stream);
    g_launches.fetch_add(1);
    g_intervals.fetch_add(intervals);
    std::vector<ScanResult> results(intervals);
    dev::hip_check(hipMemcpyAsync(results.data(), d_results, sizeof(ScanResult) * intervals, hipMemcpyDeviceToHost, r_->stream));
    dev::hip_check(hipStreamSynchronize(r_->stream));
    for (uint32_t i = 0; i + 1 < intervals; ++i)
        if (results[i].errc != kOk || (results[i].flags & seek::kSeekChecked) == 0 || (results[i].flags & seek::kSeekMismatch) != 0)
            return false;
    if (results[intervals - 1].errc != kOk)
        return false;
    copy_rows_out(destination, stride, d.pixels, row_bytes, spec.height);
    used = results[intervals - 1].bytes;
    g_scans_from_points.fetch_add(1);
    return true;
}

void ScanEngine::decode_scan_band(const ScanSpec& spec, size_t stream_offset, uint8_t* destination, size_t stride, uint32_t first_row,
                                  uint32_t rows, uint32_t lines, const uint8_t* points)
{
    ensure_stream();
    const size_t row_bytes = row_bytes_of(spec);
    const size_t point_bytes = seek_point_bytes(spec);
    const uint32_t count = points != nullptr ? seek::points_per_scan(spec.height, lines) : 0u;
    const uint32_t end = first_row + rows;
    // with seek points, every interval the band touches is a wavefront of its own (point i starts row i * lines); without,
    // one wavefront decodes from the top
    const uint32_t from = count != 0 ? std::min(first_row / lines, count) : 0u;
    const uint32_t to = count != 0 ? std::min((end - 1) / lines, count) : 0u;
    std::vector<seek::SeekWork> work;
    for (uint32_t i = from; i <= to; ++i)
    {
        seek::SeekWork w{};
        w.first_row = i * lines;
        w.end_row = i == to ? end : std::min(end, (i + 1) * lines);
        w.store_from = std::max(first_row, w.first_row);
        w.row_base = first_row;
        w.mode = seek::kResumeBand;
        w.from_point = i == 0 ? 0 : (i - 1) * point_bytes;
        work.push_back(w);
    }
    const uint32_t n = static_cast<uint32_t>(work.size());
    ScanDesc d = desc_of(spec);
    d.pixels = static_cast<uint8_t*>(r_->pixels.ensure(row_bytes * rows));
    d.pixel_stride = row_bytes;
    d.stream = r_->bits.as<uint8_t>() + stream_offset;
    d.stream_capacity = stream_bytes_ - stream_offset;
    d.line_scratch = nullptr;
    const size_t point_total = static_cast<size_t>(count) * point_bytes;
    auto* d_points = static_cast<uint8_t*>(r_->seek_points.ensure(std::max<size_t>(point_total, 16)));
    auto* d_work = static_cast<seek::SeekWork*>(r_->seek_work.ensure(dev::with_headroom(sizeof(seek::SeekWork) * n)));
    auto* d_desc = static_cast<ScanDesc*>(r_->desc.ensure(dev::with_headroom(sizeof(ScanDesc))));
    auto* d_results = static_cast<ScanResult*>(r_->result.ensure(dev::with_headroom(sizeof(ScanResult) * n)));
    if (point_total != 0)
        dev::hip_check(hipMemcpyAsync(d_points, points, point_total, hipMemcpyHostToDevice, r_->stream));
    dev::hip_check(hipMemcpyAsync(d_work, work.data(), sizeof(seek::SeekWork) * n, hipMemcpyHostToDevice, r_->stream));
    dev::hip_check(hipMemcpyAsync(d_desc, &d, sizeof d, hipMemcpyHostToDevice, r_->stream));
    dev::launch_seek_resume(d, d_desc, d_work, d_results, n, d_points, r_->stream);
    g_launches.fetch_add(1);
    g_intervals.fetch_add(n);
    std::vector<ScanResult> results(n);
    dev::hip_check(hipMemcpyAsync(results.data(), d_results, sizeof(ScanResult) * n, hipMemcpyDeviceToHost, r_->stream));
    dev::hip_check(hipStreamSynchronize(r_->stream));
    for (const ScanResult& r : results) // (the first error from the top of the band down)
        if (r.errc != kOk)
            raise(static_cast<charls_jpegls_errc>(r.errc));
    if (count != 0)
        g_scans_from_points.fetch_add(1);
    copy_rows_out(destination, stride, d.pixels, row_bytes, rows);
}

} // namespace jls
