// second_pass.inc - the ONE second pass an ingest call runs for every enabled fold (included by flowagg.hip behind
// talkers_host.inc, ports_host.inc and raw_host.inc: one translation unit).
//
// A ctx with an enabled fold - the talkers, the port tables, the flows_raw parts, or any of them together - decodes the call's n
// records again in chunks (fa_decode_device's launch on the sub-range (d_buf, len, d_off + i, m)): each chunk is decoded ONCE and
// its columns handed to every enabled fold, all on the ctx stream behind the launches of the ingest itself (ingest_device_any).
// A chunk is as long as the smallest cap of the enabled folds allows (and max_batch_records); a ctx with one fold runs what it
// ran when that fold had the pass alone.  The raw builder comes last: it waits for the stream once per chunk (raw_host.inc).

// One chunk's columns -> the enabled talker and port folds (m at most their chunk caps).  Shared by the second pass and by
// fa_raw_load (raw_load_host.inc), whose columns come out of a loaded part instead of a decode.
static int fold_chunk_cols(fa_ctx* c, const fa_columns& cols, size_t m) {
    if (c->talk) {
        const TalkCols p{cols.src_addr, cols.dst_addr, cols.etype, cols.bytes, cols.sampling_rate, cols.status, cols.time_flow_start};
        int rc = talk_fold_cols(c, p, m);
        if (rc) return rc;
    }
    if (c->ports) {
        const PortCols p{cols.src_port, cols.dst_port, cols.bytes, cols.sampling_rate, cols.time_flow_start, cols.status};
        int rc = port_fold_cols(c, p, m);
        if (rc) return rc;
    }
    return FA_OK;
}

static int second_pass_records(fa_ctx* c, const void* d_buf, size_t len, const uint32_t* d_off, size_t n) {
    for (size_t i = 0; i < n;) {
        size_t m = std::min(n - i, (size_t)c->cfg.max_batch_records);
        if (c->talk) m = std::min(m, talk_chunk_cap(c));
        if (c->ports) m = std::min(m, port_chunk_cap(c));
        if (c->raw) m = std::min(m, raw_chunk_cap(c));
        fa_columns cols;
        int rc = decode_device_records(c, d_buf, len, (size_t)((double)len * (double)m / (double)n), d_off + i, m, &cols);
        if (rc) return rc;
        rc = fold_chunk_cols(c, cols, m);
        if (rc) return rc;
        if (c->raw) {
            rc = raw_build_cols(c, cols, m);
            if (rc) return rc;
        }
        i += m;
    }
    return FA_OK;
}
