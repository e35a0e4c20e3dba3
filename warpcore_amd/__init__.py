"""warpcore_amd -- MI355X (gfx950) implementation of warpcore's per-packet
Internet / UDP checksum hot path (lib/src/in_cksum.c in the reference).

Product: ``libwccksum.so`` (HIP kernels + C ABI, ``include/warpcore_gpu``).
This package is the Python host mirror of that C ABI plus the synthetic
packet generators and the multi-GPU shard driver used by bench.py.
"""
from .cksum import (KIND_IP, KIND_PAYLOAD, SclkProbe, WcError, cksum_host, cksum_host_multi,
                    cksum_ip_udp_host, server_pause, server_paused, server_resume,
                    server_stats,
                    cksum_ip_udp_ragged, cksum_ragged_multi, gather_results_multi,
                    gpu_init_multi, shard_range,
                    cksum_ip_udp_strided, cksum_ragged, cksum_strided, gpu_init, host_register, host_unregister,
                    ip_cksum, payload_cksum, plan_strided, reload_config, synth_fill,
                    verify_ragged, verify_strided, version, shard_devices,
                    rx_verdict_ragged, rx_verdict_host, RX_NAMES, RX_DROPS,
                    RX_OK, RX_OK_NO_CKSUM, RX_BAD_IP_CKSUM, RX_BAD_UDP_CKSUM, RX_SHORT,
                    RX_FRAGMENT, RX_BAD_VERSION, RX_NOT_UDP, RX_NOT_IP, RX_TRUNCATED,
                    rx_deliver_ragged, rx_deliver_host, rx_select, rx_select_scratch,
                    RX_RECORD, RX_MASK_DELIVER, RX_MASK_HOST,
                    rx_socktab_bytes, rx_socktab_build, rx_socktab_lookup, rx_demux,
                    rx_demux_host, rx_demux_scratch, RX_SOCK, RX_SOCK_NONE, RX_SOCK_UNBOUND,
                    RX_DEMUX_MAX_SOCKS,
                    rx_engine_check, rx_reply_plan, rx_reply_build, RX_IFADDR, RX_ENGINE,
                    RX_MAX_IFADDR, RR_NAMES, RR_MASK_REPLY, RR_NONE, RR_HOST, RR_FILTERED,
                    RR_ICMP_BAD_CKSUM, RR_MALFORMED, RR_NO_ROOM, RR_ECHO4, RR_ECHO6,
                    RR_UNREACH_PORT4, RR_UNREACH_PORT6, RR_UNREACH_PROTO4,
                    tx_seal_ragged, tx_seal_host, TX_NAMES, TX_ERRORS,
                    TX_SEALED, TX_SEALED_ZERO_UDP, TX_IP_ONLY, TX_NOT_UDP, TX_NOT_IP,
                    TX_BAD_VERSION, TX_MALFORMED, TX_TRUNCATED,
                    tx_socks_check, tx_build_ragged, tx_build_host, TX_SOCK, TX_DST, TX_DESC,
                    TX_SOCK_CONNECTED, TX_SOCK_ECN, TX_BUILD_MAX_SOCKS)

__all__ = [
    "KIND_IP", "KIND_PAYLOAD", "SclkProbe", "WcError", "cksum_host", "cksum_host_multi",
    "cksum_ip_udp_host", "server_pause", "server_paused", "server_resume", "server_stats",
    "cksum_ip_udp_ragged", "cksum_ragged_multi", "gather_results_multi", "gpu_init_multi",
    "shard_range",
    "cksum_ip_udp_strided", "cksum_ragged",
    "cksum_strided", "gpu_init", "host_register", "host_unregister", "ip_cksum",
    "payload_cksum", "plan_strided", "reload_config", "synth_fill", "verify_ragged",
    "verify_strided", "version", "shard_devices", "rx_verdict_ragged", "rx_verdict_host",
    "RX_NAMES", "RX_DROPS", "RX_OK", "RX_OK_NO_CKSUM", "RX_BAD_IP_CKSUM", "RX_BAD_UDP_CKSUM",
    "RX_SHORT", "RX_FRAGMENT", "RX_BAD_VERSION", "RX_NOT_UDP", "RX_NOT_IP", "RX_TRUNCATED",
    "rx_deliver_ragged", "rx_deliver_host", "rx_select", "rx_select_scratch", "RX_RECORD",
    "RX_MASK_DELIVER", "RX_MASK_HOST",
    "rx_socktab_bytes", "rx_socktab_build", "rx_socktab_lookup", "rx_demux", "rx_demux_host",
    "rx_demux_scratch", "RX_SOCK", "RX_SOCK_NONE", "RX_SOCK_UNBOUND", "RX_DEMUX_MAX_SOCKS",
    "rx_engine_check", "rx_reply_plan", "rx_reply_build", "RX_IFADDR", "RX_ENGINE",
    "RX_MAX_IFADDR", "RR_NAMES", "RR_MASK_REPLY", "RR_NONE", "RR_HOST", "RR_FILTERED",
    "RR_ICMP_BAD_CKSUM", "RR_MALFORMED", "RR_NO_ROOM", "RR_ECHO4", "RR_ECHO6",
    "RR_UNREACH_PORT4", "RR_UNREACH_PORT6", "RR_UNREACH_PROTO4",
    "tx_seal_ragged", "tx_seal_host", "TX_NAMES", "TX_ERRORS", "TX_SEALED",
    "TX_SEALED_ZERO_UDP", "TX_IP_ONLY", "TX_NOT_UDP", "TX_NOT_IP", "TX_BAD_VERSION",
    "TX_MALFORMED", "TX_TRUNCATED",
    "tx_socks_check", "tx_build_ragged", "tx_build_host", "TX_SOCK", "TX_DST", "TX_DESC",
    "TX_SOCK_CONNECTED", "TX_SOCK_ECN", "TX_BUILD_MAX_SOCKS",
]
