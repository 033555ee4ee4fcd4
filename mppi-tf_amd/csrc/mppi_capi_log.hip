// mppi_capi_log.hip — the transition log (m_db of the reference) and its CSV writers: plain host C++, no launch. The rows are
// written by step_host (mppi_capi_step.hip), into the ring that mppi_set_transition_log sized.

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mppi_capi.hip.h"

extern "C" mppi_status mppi_set_transition_log(mppi_handle *h, int max_rows)
{
    MPPI_NOT_BATCH(h, "mppi_set_transition_log");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (max_rows < 0) return fail(h, MPPI_ERR_INVALID_ARG, "max_rows must be >= 0");
    try {
        std::vector<float> rows((size_t)max_rows * h->log_stride());
        h->log_rows.swap(rows);
    } catch (const std::bad_alloc &) {
        return fail(h, MPPI_ERR_ALLOC, "transition log: out of host memory");
    }
    h->log_cap = (size_t)max_rows; h->log_count = 0; h->log_head = 0; h->log_dropped = 0;
    return MPPI_OK;
}

extern "C" mppi_status mppi_transition_log_stats(mppi_handle *h, uint64_t *rows_held, uint64_t *rows_overwritten,
    uint64_t *rows_without_successor)
{
    MPPI_NOT_BATCH(h, "mppi_transition_log_stats");
    if (!h) return MPPI_ERR_INVALID_ARG;
    size_t open_rows = 0;
    for (size_t q = 0; q < h->log_count; ++q)
        if (h->log_rows[((h->log_head + q) % h->log_cap) * h->log_stride() + 2 * h->s + h->a] == 0.0f) ++open_rows;
    if (rows_held) *rows_held = h->log_count;
    if (rows_overwritten) *rows_overwritten = h->log_dropped;
    if (rows_without_successor) *rows_without_successor = open_rows;
    return MPPI_OK;
}

extern "C" mppi_status mppi_save_next(mppi_handle *h, const float *x_next, int n)
{
    MPPI_NOT_BATCH(h, "mppi_save_next");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x_next || n != h->s) return fail(h, MPPI_ERR_INVALID_ARG, "x_next must have s_dim floats");
    if (!h->log_cap) return MPPI_OK; // logging is off
    if (!h->log_count) return fail(h, MPPI_ERR_INVALID_ARG, "saveNext before the first next()");
    // m_db.addNext controller_base.cpp:159-163: the successor of the LAST logged (x, u) — a skipped saveNext leaves that
    // row without a successor (it is then not written) instead of shifting every later row
    float *row = h->log_rows.data() + ((h->log_head + h->log_count - 1) % h->log_cap) * h->log_stride();
    std::memcpy(row + h->s + h->a, x_next, sizeof(float) * h->s);
    row[2 * h->s + h->a] = 1.0f;
    return MPPI_OK;
}

// data_base.cpp:36-71 toCSV: header x0,..,u0,..,x_next0,.. then one row per transition, columns x | u | x_next.
// MPPI_CSV_REFERENCE writes the reference's exact bytes: every header cell and every value followed by a comma
// (tensor2CSV / csvHeader append "," after each element, so lines END with a comma), values as std::to_string(float)
// = "%f" (6 decimals). MPPI_CSV_ROUNDTRIP writes "%.9g" (fp32 round-trips) without the trailing comma.
extern "C" mppi_status mppi_to_csv_format(mppi_handle *h, const char *filename, int format)
{
    MPPI_NOT_BATCH(h, "mppi_to_csv_format");
    if (!h || !filename) return h ? fail(h, MPPI_ERR_INVALID_ARG, "filename is NULL") : MPPI_ERR_INVALID_ARG;
    if (format != MPPI_CSV_REFERENCE && format != MPPI_CSV_ROUNDTRIP) return fail(h, MPPI_ERR_INVALID_ARG, "unknown CSV format");
    if (!h->log_cap) return fail(h, MPPI_ERR_INVALID_ARG, "the transition log is off: call mppi_set_transition_log first");
    FILE *f = std::fopen(filename, "w");
    if (!f) return fail(h, MPPI_ERR_IO, std::string("cannot open ") + filename);
    const bool ref = format == MPPI_CSV_REFERENCE;
    const int s = h->s, a = h->a;
    for (int i = 0; i < s; ++i) std::fprintf(f, "x%d,", i);
    for (int i = 0; i < a; ++i) std::fprintf(f, "u%d,", i);
    for (int i = 0; i < s; ++i) std::fprintf(f, (ref || i + 1 < s) ? "x_next%d," : "x_next%d", i);
    std::fputc('\n', f);
    for (size_t q = 0; q < h->log_count; ++q) {
        const float *row = h->log_rows.data() + ((h->log_head + q) % h->log_cap) * h->log_stride();
        if (row[2 * s + a] == 0.0f) continue; // no successor recorded
        const int n = 2 * s + a;
        for (int i = 0; i < n; ++i) {
            if (ref) std::fprintf(f, "%f,", (double)row[i]); // std::to_string(float)
            else std::fprintf(f, i + 1 < n ? "%.9g," : "%.9g", (double)row[i]);
        }
        std::fputc('\n', f);
    }
    if (std::fclose(f) != 0) return fail(h, MPPI_ERR_IO, std::string("write failed: ") + filename);
    return MPPI_OK;
}

// replaces ControllerBase::toCSV (controller_base.cpp:164): the reference's format
extern "C" mppi_status mppi_to_csv(mppi_handle *h, const char *filename) { return mppi_to_csv_format(h, filename, MPPI_CSV_REFERENCE); }
