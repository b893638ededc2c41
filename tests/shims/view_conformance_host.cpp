// TEST INFRASTRUCTURE.  Host half of the world view API conformance check (see
// view_conformance.inl): plain host C++, as a simulator's Manager is.
#define VIEWCONF_NAME viewconf_host
#include "view_conformance.inl"
